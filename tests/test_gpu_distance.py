"""GPU: the occupancy distance field (include/loamx.h, "occupancy distance field"; loam_amd/csrc/distance_kernels.hip) against the
brute-force numpy model of tests/distance_common.py, by equality of bytes: squared distances, offsets and metres of a box or a
slice. Outputs are poisoned before every call and the entries behind their ends must stay poison. Every comparison is made in both
forms of the y- and z-pass (context option NO_DISTANCE_EARLY_EXIT), which must leave the same bytes. Obstacles at chosen voxels
come from one ray per voxel that never leaves it (distance_common.place_rays), so the named cases are those the g++ build of
distance_math.h is compared on (test_distance_hostcheck.py)."""
import ctypes as C

import numpy as np
import pytest

import crop_common as X
import distance_common as D
import occupancy_common as M
import outdoor_scenes as S
from gpu_common import ctx, option
from loam_amd import capi

pytestmark = pytest.mark.gpu

POISON = 0xA5
PAD = 5  # entries behind every output that must stay poison
LEAF = 0.2


def make(max_voxels=1 << 14, **params):
    return ctx().occupancy_map(capi.OccupancyParams(**params), max_voxels), M.OccupancyModel(**params)


def dev_add(m, pts, offsets=None, poses=None):
    c = m.ctx
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    offsets = [0, len(pts)] if offsets is None else offsets
    d_pts = c.alloc(max(pts.nbytes, 8))
    d_poses = c.alloc(max(np.asarray(poses).nbytes, 8)) if poses is not None else None
    try:
        if pts.size:
            d_pts.upload(pts)
        if poses is not None:
            d_poses.upload(np.ascontiguousarray(poses, dtype=np.float64))
        m.add_clouds_dev(d_pts.ptr, 3, offsets, d_poses.ptr if d_poses else 0)
        c.synchronize()
    finally:
        d_pts.free()
        if d_poses:
            d_poses.free()


def placed(voxels, leaf=LEAF, **params):
    """a map and its model with exactly the given voxels OCCUPIED (one hit each) and nothing else in the table"""
    m, model = make(leaf=leaf, **dict(D.PLACE, **params))
    voxels = np.asarray(voxels, dtype=np.int64).reshape(-1, 3)
    if len(voxels):
        pts, offsets, poses = D.place_rays(voxels, leaf)
        dev_add(m, pts, offsets, poses)
        model.add(pts, offsets, poses)
    want = {tuple(v) for v in voxels.tolist()}
    assert {tuple(v) for v in M.key_coords(list(model.vox)).tolist()} == want if want else not model.vox
    assert all(c == [1, 0] for c in model.vox.values())
    return m, model


def _poisoned(c, nbytes):
    return c.alloc(nbytes).upload(np.full(nbytes, POISON, dtype=np.uint8))


def dev_field(m, vmin, dims, params, slice2d=False, want=(True, True, True)):
    """the device form into poisoned buffers of n + PAD entries -> (d2, offset, metres), None for an output that was not asked
    for; what was not asked for and everything behind the ends must still be poison"""
    c = m.ctx
    axes = 2 if slice2d else 3
    shape = (int(dims[1]), int(dims[0])) if slice2d else (int(dims[2]), int(dims[1]), int(dims[0]))
    n = int(np.prod(shape))
    sizes = (2, 2 * axes, 4)
    bufs = [_poisoned(c, (n + PAD) * s) for s in sizes]
    try:
        fn = m.distance_slice_dev if slice2d else m.distance_box_dev
        fn(vmin, dims, params, *[b.ptr if w else 0 for b, w in zip(bufs, want)])
        c.synchronize()
        raw = [b.download(np.uint8, (n + PAD) * s) for b, s in zip(bufs, sizes)]
    finally:
        for b in bufs:
            b.free()
    out = []
    for r, s, w, dtype, shp in zip(raw, sizes, want, (np.uint16, np.int16, np.float32), (shape, shape + (axes,), shape)):
        assert (r[n * s if w else 0:] == POISON).all(), "written past the end, or an output that was not asked for"
        out.append(r[:n * s].copy().view(dtype).reshape(shp) if w else None)
    return tuple(out)


def assert_same(got, want, what):
    for name, g, w in zip(("d2", "offset", "metres"), got, want):
        assert g.shape == w.shape and D.same_bytes(g, w), (what, name)


def check(m, model, vmin, dims, R, unknown=False, slice2d=False, what=""):
    """both option forms against the model; returns the model's field"""
    want = D.model_field(model, vmin, dims, R, unknown, slice2d)
    params = capi.DistanceParams(R, int(unknown))
    for whole in (0, 1):
        with option("NO_DISTANCE_EARLY_EXIT", whole):
            assert_same(dev_field(m, vmin, dims, params, slice2d), want, (what, "whole window" if whole else "early exit"))
    return want


# ---- 1. the named cases: mask words, the cap, ties, the stop rule's edge, the halo, dims of one, negative vmin ----------------------
CASES = D.named_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_named_cases_in_both_forms(name):
    case = CASES[name]
    slice2d = bool(case.get("slice"))
    m, model = placed(case["obst"])
    try:
        want = check(m, model, case["vmin"], case["dims"], case["R"], slice2d=slice2d, what=name)
        assert_same(want, D.case_field(case, LEAF), (name, "the model from the map's states equals the model from the list"))
    finally:
        m.close()


# ---- 2. empty map -------------------------------------------------------------------------------------------------------------------
def test_an_empty_map_is_far_everywhere_or_zero_everywhere():
    m, model = make(leaf=LEAF)
    try:
        for slice2d in (False, True):
            d2, off, metres = check(m, model, (-3, 2, -1), (7, 5, 3), 4, slice2d=slice2d, what="empty")
            assert (d2 == D.FAR).all() and not off.any() and np.isposinf(metres).all()
            d2, off, metres = check(m, model, (-3, 2, -1), (7, 5, 3), 4, unknown=True, slice2d=slice2d, what="empty, unknown")
            assert not d2.any() and not off.any() and not metres.any()
    finally:
        m.close()


def test_voxels_outside_the_key_range_are_unknown_and_so_obstacles():
    """a corridor of FREE voxels that ends in a hit at |v| = 2^20 - 1; the box and its halo reach beyond the range on every axis"""
    leaf, B = 0.5, M.BIAS
    m, model = make(leaf=leaf)
    pose = np.array([[0.0, 0.0, 0.0, 1.0, (B - 6 + 0.5) * leaf, (B - 1 + 0.5) * leaf, (1.5 - B) * leaf]])
    pts = np.array([[5 * leaf, 0.0, 0.0]])
    try:
        dev_add(m, pts, poses=pose)
        model.add(pts, poses=pose)
        states = model.box((B - 6, B - 1, -B + 1), (6, 1, 1))[1].ravel().tolist()
        assert states == [M.FREE] * 5 + [M.OCCUPIED]
        for R in (1, 4):
            vmin, dims = (B - 7, B - 3, -B - 1), (9, 5, 4)
            d2, _, _ = check(m, model, vmin, dims, R, unknown=True, what=("range edge", R))
            assert d2[2, 2, 1:6].tolist() == [1] * 5 and d2[2, 2, 6] == 0 and d2[2, 2, 7] == 0  # the free corridor: its neighbours are unknown
            check(m, model, vmin, dims, R, unknown=True, slice2d=True, what=("range edge, slice", R))
            d2, _, _ = check(m, model, vmin, dims, R, what=("range edge, occupied only", R))
            assert d2[2, 2, 6] == 0 and d2[2, 2, 5] == 1 and ((d2 != D.FAR).sum() > 7) == (R > 1)
    finally:
        m.close()


# ---- 3. slices ------------------------------------------------------------------------------------------------------------------------
def test_slices_take_their_columns_over_the_levels_they_are_given():
    obst = [(2, 2, 4), (5, 1, 4), (0, 0, 0), (7, 3, 2), (-2, 4, 1), (12, 0, 4)]  # (two of them in the halo)
    m, model = placed(obst)
    try:
        fields = {}
        for levels in (1, 3, 5):
            d2, off, _ = fields[levels] = check(m, model, (0, 0, 0), (9, 6, levels), 4, slice2d=True, what=("levels", levels))
            assert (d2[0, 0] == 0) and (d2[3, 7] == 0) == (levels >= 3) and (d2[2, 2] == 0) == (levels == 5)
        assert fields[5][0][0, 8] == 10 and fields[5][1][0, 8].tolist() == [-3, 1]  # (5, 1) and (7, 3) tie at 10: the lower y
        assert fields[3][0][4, 0] == 4 and fields[3][1][4, 0].tolist() == [-2, 0]   # the halo's column (-2, 4), seen from level 1 on
        assert fields[1][0][4, 0] == 16 and fields[1][1][4, 0].tolist() == [0, -4]  # one level: only (0, 0) is left, at the cap
        for levels in (1, 5):
            d2, _, _ = check(m, model, (0, 0, 0), (9, 6, levels), 4, unknown=True, slice2d=True, what=("levels, unknown", levels))
            assert not d2.any()  # every column is OCCUPIED or all-unknown
        d2, _, _ = check(m, model, (0, 0, 0), (9, 6, 0), 4, slice2d=True, what="no levels")
        assert (d2 == D.FAR).all()
    finally:
        m.close()


def scene(seed, **params):
    pts, pose = M.random_rays(seed, 1500, 5.0)
    m, model = make(1 << 17, leaf=0.25, **params)
    dev_add(m, pts, poses=pose[None])
    model.add(pts, poses=pose[None])
    return m, model, np.floor(pose[4:] / 0.25).astype(np.int64)


def test_a_scene_of_rays_as_box_and_slice_under_both_settings_of_unknown():
    m, model, sensor = scene(51)
    try:
        lo, dims = model.bounds()
        for levels in (1, 5):
            vmin, d = np.array([lo[0], lo[1], sensor[2] - levels // 2]), np.array([dims[0], dims[1], levels])
            d2, _, _ = check(m, model, vmin, d, 6, slice2d=True, what=("scene slice", levels))
            assert (d2 == 0).any() and (d2 == D.FAR).any() and ((d2 > 0) & (d2 < D.FAR)).sum() > 200
            d2u, _, _ = check(m, model, vmin, d, 6, unknown=True, slice2d=True, what=("scene slice, unknown", levels))
            assert (d2u <= d2).all() and (d2u < d2).any() and (d2u > 0).any()
        vmin, d = sensor - [6, 5, 3], np.array([12, 10, 6])
        d2, _, _ = check(m, model, vmin, d, 3, what="scene box")
        d2u, _, _ = check(m, model, vmin, d, 3, unknown=True, what="scene box, unknown")
        assert (d2u <= d2).all() and (d2u > 0).any()
        vmin, d = np.array([lo[0], lo[1], sensor[2] - 2]), np.array([dims[0], dims[1], 4])
        d2, _, _ = check(m, model, vmin, d, 9, what="scene box over the whole footprint")
        assert (d2 == 0).sum() > 50 and ((d2 > 0) & (d2 < D.FAR)).sum() > 1000
    finally:
        m.close()


# ---- 4. the state rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thresholds", [dict(min_hits=2, occ_ratio=0.0, min_passes=3), dict(min_hits=1, occ_ratio=0.5, min_passes=1),
                                        dict(min_hits=0, occ_ratio=0.0, min_passes=0)])
def test_the_field_follows_the_maps_thresholds(thresholds):
    m, model, sensor = scene(52, **thresholds)
    plain = M.OccupancyModel(leaf=0.25)
    pts, pose = M.random_rays(52, 1500, 5.0)
    plain.add(pts, poses=pose[None])
    try:
        lo, dims = model.bounds()
        vmin, d = np.array([lo[0], lo[1], sensor[2] - 1]), np.array([dims[0], dims[1], 3])
        if thresholds["min_hits"] == 0:  # 0 hits >= 0: every voxel is OCCUPIED, a voxel without a slot included
            d2, _, _ = check(m, model, sensor - 2, (5, 4, 3), 2, what=thresholds)
            assert not d2.any()
            assert not check(m, model, sensor - 2, (5, 4, 3), 2, slice2d=True, what=thresholds)[0].any()
            return
        d2, _, _ = check(m, model, vmin, d, 5, slice2d=True, what=thresholds)
        base = D.model_field(plain, vmin, d, 5, slice2d=True)[0]
        assert (d2 >= base).all() and (d2 > base).any() and (d2 == 0).any()  # passes erase hits: fewer obstacles, larger distances
        check(m, model, vmin, d, 5, unknown=True, slice2d=True, what=(thresholds, "unknown"))
        check(m, model, sensor - [6, 5, 2], (12, 10, 4), 3, what=(thresholds, "box"))
    finally:
        m.close()


# ---- 5. staging, optional outputs ---------------------------------------------------------------------------------------------------
def test_the_staging_grows_with_the_call_and_serves_smaller_calls_again():
    m, model, sensor = scene(53)
    try:
        lo, dims = model.bounds()
        small = (sensor - 2, np.array([5, 4, 3]), 2)
        large = (lo, np.array([dims[0], dims[1], 6]), 7)
        first = check(m, model, *small, what="small")
        check(m, model, *small, slice2d=True, what="small slice")
        check(m, model, *large, what="large")
        check(m, model, *large, slice2d=True, what="large slice")
        assert_same(check(m, model, *small, what="small again"), first, "small again")
        M.assert_stats_equal(m.stats(), model.stats(), "the table is only read")
    finally:
        m.close()


@pytest.mark.parametrize("slice2d", [False, True])
def test_each_output_may_be_left_out(slice2d):
    m, model = placed([(1, 1, 1), (4, 2, 0), (-2, 0, 1)])
    try:
        vmin, dims, R = (0, 0, 0), (6, 4, 2), 3
        want = D.model_field(model, vmin, dims, R, False, slice2d)
        params = capi.DistanceParams(R)
        for asked in ((False, True, True), (True, False, True), (True, True, False), (True, False, False), (False, False, True), (False, False, False)):
            got = dev_field(m, vmin, dims, params, slice2d, asked)
            for g, w, a in zip(got, want, asked):
                assert (g is None) if not a else D.same_bytes(g, w), asked
    finally:
        m.close()


def test_the_host_forms_equal_the_device_forms():
    m, model, sensor = scene(54)
    try:
        vmin, dims = sensor - [6, 5, 2], (12, 10, 4)
        for unknown in (0, 1):
            p = capi.DistanceParams(3, unknown)
            assert_same(m.distance_box(vmin, dims, p), D.model_field(model, vmin, dims, 3, bool(unknown)), ("host box", unknown))
            assert_same(m.distance_slice(vmin, dims, p), D.model_field(model, vmin, dims, 3, bool(unknown), True), ("host slice", unknown))
        got = m.distance_box(vmin, (12, 0, 4))
        assert got[0].shape == (4, 0, 12) and got[1].shape == (4, 0, 12, 3)
        d = capi.DistanceParams()
        assert (d.max_dist_voxels, d.unknown_is_obstacle, capi.DIST_FAR) == (10, 0, D.FAR)
    finally:
        m.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def status_of(fn, *args, **kw):
    try:
        fn(*args, **kw)
        return capi.OK
    except capi.LoamxError as e:
        return e.status


def test_refusals_change_nothing():
    c = ctx()
    m, model, sensor = scene(55)
    other = capi.Context(0)
    d_out = _poisoned(c, 4096)
    o = d_out.ptr
    try:
        vmin, dims = sensor - 2, np.array([4, 3, 2])
        before = (check(m, model, vmin, dims, 3, what="before"), m.stats().tobytes(), m.claims())
        lib = c.lib
        v3, d3 = (C.c_int32 * 3)(0, 0, 0), (C.c_uint32 * 3)(2, 2, 2)
        p = capi.DistanceParams(3).struct()
        for name in ("loamx_occupancy_distance_box", "loamx_occupancy_distance_slice"):
            fn = getattr(lib, name)
            assert fn(c.h, None, v3, d3, C.byref(p), o, o, o) == capi.ERR_BAD_PARAM
            assert fn(c.h, m.h, None, d3, C.byref(p), o, o, o) == capi.ERR_BAD_PARAM
            assert fn(c.h, m.h, v3, None, C.byref(p), o, o, o) == capi.ERR_BAD_PARAM
            assert fn(c.h, m.h, v3, d3, None, o, o, o) == capi.ERR_BAD_PARAM
            assert fn(None, m.h, v3, d3, C.byref(p), o, o, o) == capi.ERR_BAD_PARAM
            assert fn(other.h, m.h, v3, d3, C.byref(p), o, o, o) == capi.ERR_BAD_PARAM  # a map of another context
        host = np.full(64, POISON, dtype=np.uint8)
        for name in ("loamx_occupancy_distance_box_host", "loamx_occupancy_distance_slice_host"):
            fn = getattr(lib, name)
            assert fn(c.h, m.h, v3, d3, None, host.ctypes.data, host.ctypes.data, host.ctypes.data) == capi.ERR_BAD_PARAM
            assert fn(other.h, m.h, v3, d3, C.byref(p), host.ctypes.data, host.ctypes.data, host.ctypes.data) == capi.ERR_BAD_PARAM
        assert (host == POISON).all()
        for fn in (m.distance_box_dev, m.distance_slice_dev):
            assert status_of(fn, vmin, dims, capi.DistanceParams(0), o, o, o) == capi.ERR_BAD_PARAM
            assert status_of(fn, vmin, dims, capi.DistanceParams(256), o, o, o) == capi.ERR_UNSUPPORTED
        # the EXTENDED box decides: 2^31 voxels pass the box's own test and fail with the halo
        assert status_of(m.distance_box_dev, vmin, [1 << 11, 1 << 11, 1 << 9], capi.DistanceParams(1), o, o, o) == capi.ERR_UNSUPPORTED
        assert status_of(m.distance_slice_dev, vmin, [1 << 16, 1 << 15, 1], capi.DistanceParams(1), o, o, o) == capi.ERR_UNSUPPORTED
        assert status_of(m.distance_box_dev, vmin, [0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF], capi.DistanceParams(255), o, o, o) == capi.ERR_UNSUPPORTED
        assert status_of(m.distance_slice_dev, vmin, [0xFFFFFFFF, 0xFFFFFFFF, 0], capi.DistanceParams(255), o, o, o) == capi.ERR_UNSUPPORTED
        assert status_of(m.distance_box_dev, vmin, [0, 0xFFFFFFFF, 3], capi.DistanceParams(4), o, o, o) == capi.ERR_UNSUPPORTED  # (0 + 2R) x 2^32
        c.synchronize()
        assert (d_out.download(np.uint8, 4096) == POISON).all()  # a refused call writes nothing
        # nothing to do is not a refusal
        assert status_of(m.distance_box_dev, vmin, [3, 0, 3], capi.DistanceParams(2), o, o, o) == capi.OK
        assert status_of(m.distance_box_dev, vmin, [3, 3, 0], capi.DistanceParams(2), o, o, o) == capi.OK
        assert status_of(m.distance_slice_dev, vmin, [0, 5, 2], capi.DistanceParams(2), o, o, o) == capi.OK
        assert status_of(m.distance_box_dev, vmin, dims, capi.DistanceParams(2), 0, 0, 0) == capi.OK
        c.synchronize()
        assert (d_out.download(np.uint8, 4096) == POISON).all()
        after = (check(m, model, vmin, dims, 3, what="after"), m.stats().tobytes(), m.claims())
        assert_same(after[0], before[0], "after the refusals")
        assert after[1:] == before[1:]
        with pytest.raises(ValueError):
            m.distance_box_dev([0, 0], [1, 1, 1], None, o, o, o)
    finally:
        d_out.free(), other.close(), m.close()
    with pytest.raises(ValueError):
        m.distance_box_dev(vmin, dims, None, 0, 0, 0)  # closed


# ---- 7. after a crop ------------------------------------------------------------------------------------------------------------------
def test_the_field_of_a_cropped_map_is_the_cropped_models():
    m, model, sensor = scene(56)
    try:
        lo, dims = model.bounds()
        vmin, d = np.array([lo[0], lo[1], sensor[2] - 1]), np.array([dims[0], dims[1], 3])
        before = check(m, model, vmin, d, 6, slice2d=True, what="before the crop")[0]
        centre = (sensor + 0.5) * 0.25
        kept, removed = m.crop([-2.0, -2.0, -1.0], [2.0, 2.0, 1.0], centre)
        got = X.crop_model(model, np.concatenate([[0, 0, 0, 1.0], centre]), [-2.0, -2.0, -1.0], [2.0, 2.0, 1.0])
        assert (kept, removed) == got[:2] and kept > 100 and removed > 100
        after = check(m, model, vmin, d, 6, slice2d=True, what="after the crop")[0]
        assert (after >= before).all() and (after > before).any() and (after == 0).any()
        check(m, model, sensor - [10, 9, 2], (20, 18, 4), 4, what="box after the crop")
        check(m, model, sensor - [6, 5, 2], (12, 10, 4), 2, unknown=True, what="box after the crop, unknown")
    finally:
        m.close()


# ---- 8. an organised scan -----------------------------------------------------------------------------------------------------------
def _cells_in_front_of_walls(d2, off, grid, sx, sy):
    """along the four grid directions from the sensor's cell: the FREE cells directly in front of the first OCCUPIED cell. Returns
    how many of them read k^2 with the offset pointing at that wall cell, k = 1, 2, ... as far as nothing else is nearer."""
    found = 0
    for ddx, ddy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        x, y, run = sx, sy, []
        while 0 <= x < grid.shape[1] and 0 <= y < grid.shape[0] and grid[y, x] != M.OCCUPIED:
            run.append((x, y))
            x, y = x + ddx, y + ddy
        if not (0 <= x < grid.shape[1] and 0 <= y < grid.shape[0]):
            continue
        assert d2[y, x] == 0  # the wall cell
        for k, (cx, cy) in enumerate(reversed(run), start=1):
            if grid[cy, cx] != M.FREE or d2[cy, cx] != k * k:
                break
            if off[cy, cx].tolist() == [ddx * k, ddy * k]:
                found += 1
    return found


def test_an_organised_lot_scan_becomes_a_clearance_grid():
    import organize_common as OC
    c = ctx()
    H, W = 16, 256
    origin, yaw = S.sensor_origin("lot", 0)
    scan = S.scan_at("lot", 0, origin, yaw, H=H, W=W)
    cloud = scan[np.random.default_rng(28).permutation(H * W)]
    lidar = capi.LidarParams(H, W, 1.0, 120.0)
    lay = c.scan_layout(lidar, capi.OrganizeParams(elevations=OC.fan_elevations(H, S.FANS["lot"])))
    results = np.zeros(2, dtype=capi.RESULT_DTYPE)
    results["pose"] = [S.yaw_pose(0.3, [1.5, 0.2, 0.0]), S.yaw_pose(-0.1, [1.0, -0.3, 0.05])]
    leaf, R = 0.4, 12
    m, model = make(max_voxels=1 << 18, leaf=leaf, max_range=40.0)
    bufs = [c.alloc(cloud.nbytes).upload(cloud), c.alloc(H * W * 24), c.alloc(results.nbytes).upload(results), c.alloc(3 * 56)]
    d_cloud, d_scan, d_results, d_traj = bufs
    try:
        c.organize_clouds_dev(lay, d_cloud.ptr, 3, [0, H * W], d_scan.ptr)
        c.compose_trajectory_dev(d_results.ptr, 2, d_traj.ptr, origin=S.yaw_pose(yaw, origin))
        m.add_clouds_dev(d_scan.ptr, 3, [0, H * W], d_traj.ptr + 2 * 56)
        c.synchronize()
        organised = d_scan.download(np.float64, H * W * 3).reshape(-1, 3)
        traj = d_traj.download(np.float64, 21).reshape(3, 7)
        model.add(organised, poses=traj[2:3])
        lo, dims = model.bounds()
        sensor = np.floor(traj[2, 4:] / leaf).astype(np.int64)
        vmin, d = np.array([lo[0], lo[1], sensor[2] - 1], dtype=np.int32), np.array([dims[0], dims[1], 3], dtype=np.uint32)
        grid = model.slice(vmin, d)
        sx, sy = int(sensor[0] - lo[0]), int(sensor[1] - lo[1])
        want = D.model_field(model, vmin, d, R, slice2d=True)
        # the scene first, on the model: wall cells are 0 and nothing else is, and FREE cells in front of a wall read k^2 towards it
        assert grid[sy, sx] == M.FREE and ((want[0] == 0) == (grid == M.OCCUPIED)).all() and (grid == M.OCCUPIED).sum() > 50
        assert _cells_in_front_of_walls(want[0], want[1], grid, sx, sy) >= 2
        near = (want[0] > 0) & (want[0] < D.FAR)
        assert near.sum() > 500 and (want[2][near] == (np.sqrt(want[0][near].astype(np.float64)) * leaf).astype(np.float32)).all()
        assert np.isposinf(want[2][want[0] == D.FAR]).all() and (want[0] == D.FAR).any()
        # ... then the kernels
        check(m, model, vmin, d, R, slice2d=True, what="lot")
    finally:
        for b in bufs:
            b.free()
        m.close(), lay.close()
