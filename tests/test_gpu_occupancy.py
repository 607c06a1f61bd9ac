"""GPU: the occupancy map (include/loamx.h, "occupancy map"; loam_amd/csrc/occupancy_kernels.hip) against the numpy model of
tests/occupancy_common.py, by equality of bytes: the counts and states of a dense box over the model's bounding box, of a query
at every voxel of the model, and the stats. Outputs are poisoned before every read-out. Run combining and the plain
one-visit-one-claim form (context option NO_OCCUPANCY_COMBINE) must leave the same bytes; `claims` tells them apart."""
import ctypes as C

import numpy as np
import pytest

import cloudmap_common as CM
import occupancy_common as M
import outdoor_scenes as S
from gpu_common import ctx, option
from loam_amd import capi
from map_common import small_pose

pytestmark = pytest.mark.gpu

POISON = 0xA5
POISON_U32 = np.uint32(0xA5A5A5A5)
PAD = 5  # entries behind every output that must stay poison


def dev_add(m, pts, offsets=None, poses=None):
    """uploads the clouds and their poses and adds them through the device entry point (one call)"""
    c = m.ctx
    pts = np.ascontiguousarray(pts)
    assert pts.ndim == 2 and pts.dtype in (np.float32, np.float64)
    offsets = [0, len(pts)] if offsets is None else offsets
    d_pts = c.alloc(max(pts.nbytes, 8))
    d_poses = c.alloc(max(np.asarray(poses).nbytes, 8)) if poses is not None else None
    try:
        if pts.size:
            d_pts.upload(pts)
        if poses is not None:
            d_poses.upload(np.ascontiguousarray(poses, dtype=np.float64))
        m.add_clouds_dev(d_pts.ptr, pts.shape[1], offsets, d_poses.ptr if d_poses else 0, f32=pts.dtype == np.float32)
        c.synchronize()
    finally:
        d_pts.free()
        if d_poses:
            d_poses.free()


def _poisoned(c, nbytes):
    return c.alloc(nbytes).upload(np.full(nbytes, POISON, dtype=np.uint8))


def _read(fn, c, n, with_counts=True, with_state=True):
    """fn(d_counts, d_state) into poisoned buffers of n + PAD entries; (counts (n, 2) or None, state (n,) or None) after checking
    that nothing else was written"""
    bufs = [_poisoned(c, (n + PAD) * 8), _poisoned(c, n + PAD)]
    try:
        fn(bufs[0].ptr if with_counts else 0, bufs[1].ptr if with_state else 0)
        c.synchronize()
        counts, state = bufs[0].download(np.uint32, (n + PAD) * 2).reshape(-1, 2), bufs[1].download(np.uint8, n + PAD)
    finally:
        for b in bufs:
            b.free()
    assert (counts[n if with_counts else 0:] == POISON_U32).all() and (state[n if with_state else 0:] == POISON).all(), "written past the end"
    return counts[:n].copy() if with_counts else None, state[:n].copy() if with_state else None


def dev_box(m, vmin, dims, **kw):
    n = int(np.prod(np.asarray(dims, dtype=np.int64)))
    counts, state = _read(lambda dc, ds: m.box_dev(vmin, dims, dc, ds), m.ctx, n, **kw)
    shape = (int(dims[2]), int(dims[1]), int(dims[0]))
    return None if counts is None else counts.reshape(shape + (2,)), None if state is None else state.reshape(shape)


def dev_query(m, pts, stride=3, **kw):
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    d_pts = m.ctx.alloc(max(pts.nbytes, 8))
    try:
        if pts.size:
            d_pts.upload(pts)
        return _read(lambda dc, ds: m.query_dev(d_pts.ptr, stride, len(pts), dc, ds), m.ctx, len(pts), **kw)
    finally:
        d_pts.free()


def dev_slice(m, vmin, dims):
    n = int(dims[0]) * int(dims[1])
    buf = _poisoned(m.ctx, n + PAD)
    try:
        m.slice_dev(vmin, dims, buf.ptr)
        m.ctx.synchronize()
        grid = buf.download(np.uint8, n + PAD)
    finally:
        buf.free()
    assert (grid[n:] == POISON).all()
    return grid[:n].reshape(int(dims[1]), int(dims[0])).copy()


def snapshot(m, vmin, dims):
    return dev_box(m, vmin, dims) + (m.stats().tobytes(), m.claims())


def check(m, model, what=""):
    """box over the model's bounding box, query at the model's voxels and a few points elsewhere, stats"""
    M.assert_stats_equal(m.stats(), model.stats(), what)
    if not model.vox:
        return None
    vmin, dims = model.bounds()
    counts, state = dev_box(m, vmin, dims)
    want = model.box(vmin, dims)
    assert M.same_bytes(counts, want[0]), (what, "box counts")
    assert M.same_bytes(state, want[1]), (what, "box states")
    assert int(counts[..., 0].sum()) == int(model.stats()["rays_hit"]) and int(counts[..., 1].sum()) == int(model.stats()["visits"]), what
    leaf = model.p["leaf"]
    centres = (M.key_coords(list(model.vox)[:4000]) + 0.5) * leaf
    pts = np.concatenate([centres, centres[:50] + 1000.0 * leaf, [[np.nan, 0, 0], [0, 0, 2e6 * leaf]]])
    q = dev_query(m, pts)
    want = model.query(pts)
    assert M.same_bytes(q[0], want[0]) and M.same_bytes(q[1], want[1]), (what, "query")
    return counts, state


def make(max_voxels=1 << 17, **params):
    return ctx().occupancy_map(capi.OccupancyParams(**params), max_voxels), M.OccupancyModel(**params)


def both_forms(params, pts, offsets=None, poses=None, what="", max_voxels=1 << 17):
    """the same call through both kernel forms: each equals the model, the claims are the model's for that form"""
    results = []
    for plain in (0, 1):
        m, model = make(max_voxels, **params)
        try:
            with option("NO_OCCUPANCY_COMBINE", plain):
                dev_add(m, pts, offsets, poses)
            model.add(pts, offsets, poses)
            results.append(check(m, model, (what, plain)))
            assert m.claims() == (model.plain_claims if plain else model.wave_claims), (what, plain, m.claims(), model.plain_claims, model.wave_claims)
        finally:
            m.close()
    if results[0] is not None:
        assert M.same_bytes(results[0][0], results[1][0]) and M.same_bytes(results[0][1], results[1][1]), what
    return model


# ---- 1. the walk -------------------------------------------------------------------------------------------------------------
CASES = M.walk_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_edges_of_the_rule_in_both_forms(name):
    p, pts, pose = CASES[name]
    model = both_forms(p, pts, poses=None if pose is None else pose[None], what=name)
    st = model.stats()
    if name.startswith("voxel_range_") and "last_voxel" not in name and name not in M.WALK_END_CASES:
        assert st["outside"] > 0
    if name in M.WALK_END_CASES:  # the walk end alone decides: one long ray is outside and leaves nothing, or none is
        lost = M.WALK_END_CASES[name][0]
        assert (st["outside"], st["rays_hit"], st["range_long"]) == (0 if lost is None else 1, 0, 3)
        r = M.Rays(pts, pose, p["leaf"], p["min_range"], p["max_range"], p["end_margin"], 1)
        assert r.walks.tolist() == [i != lost for i in range(3)] and st["visits"] == int((r.steps + 1)[r.walks].sum())
    if name.startswith("ranges_"):
        assert (st["invalid"], st["range_short"], st["range_long"]) == (4, 3, 4) and st["rays_hit"] == 5


# ---- 2. runs -----------------------------------------------------------------------------------------------------------------
def run_patterns():
    a, b = [7.3, 2.1, 0.4], [-3.2, 6.6, 1.7]
    out = {}
    out["one_run_of_64"] = np.tile([a], (64, 1))
    out["one_ray_320_times"] = np.tile([a], (320, 1))  # runs end at lanes 63 / 64 and at the workgroup's edge
    out["a_b_a"] = np.array([a, b, a] * 30)
    p = np.tile([a], (100, 1))
    p[[5, 40, 41, 70]] = [[np.nan, 0, 0], [0, 0, 0], [500.0, 0, 0], [0.01, 0, 0]]  # invalid, short, long (walks on), short
    out["runs_broken_by_dropped_lanes"] = p
    near, one, far = [0.012, 0.011, 0.013], [0.13, 0.02, 0.02], [40.0, 0.03, 0.02]
    out["0_1_and_400_steps_side_by_side"] = np.array([near, one, far, far, near, one, near, far] * 9)
    return out


PATTERNS = run_patterns()


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_runs_inside_and_across_wavefronts_combined_and_plain(name):
    pts = PATTERNS[name]
    params = dict(leaf=0.1, min_range=0.015, end_margin=0.0) if name.startswith("0_1") else dict(leaf=0.5, min_range=0.1, max_range=20.0)
    model = both_forms(params, pts, what=name)
    if name == "one_run_of_64":
        assert model.wave_claims * 64 == model.plain_claims
    if name == "a_b_a":
        assert model.wave_claims > model.plain_claims // 2  # only the shared start of the two walks combines
    if name.startswith("0_1"):
        r = M.Rays(pts[:3], None, 0.1, 0.015, 80.0, 0.0, 1)
        assert r.steps.tolist() == [0, 1, 400] and r.walks.all()


# ---- 3. storage and calls ------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 63, 64, 0, 65, 255, 256, 257, 1000, 0)  # an empty cloud first, in the middle and last


def clouds(seed, reach=6.0):
    rng = np.random.default_rng(seed)
    pts, _ = M.random_rays(seed, sum(SIZES), reach)
    offsets = np.concatenate([[0], np.cumsum(SIZES)])
    poses = np.stack([small_pose(rng, angle=0.8, shift=3.0) for _ in SIZES])
    return pts, offsets, poses


@pytest.mark.parametrize("dtype,stride,posed", [(np.float64, 3, True), (np.float64, 5, False), (np.float32, 3, False), (np.float32, 5, True)])
def test_clouds_of_every_size_in_one_batch(dtype, stride, posed):
    xyz, offsets, poses = clouds(31)
    pts = np.full((len(xyz), stride), np.nan)  # (the scalars behind z are never read)
    pts[:, :3] = xyz
    pts = pts.astype(dtype)
    model = both_forms(dict(leaf=0.25, max_range=5.0), pts, offsets, poses if posed else None, what=(dtype, stride, posed))
    st = model.stats()
    assert st["range_long"] > 100 and st["rays_hit"] > 1000 and st["visits"] > 20 * st["rays_hit"] and st["voxels"] > 5000


def test_offsets_that_do_not_start_at_zero_count_from_the_first_offset():
    pts, _ = M.random_rays(32, 700, 5.0)
    m, model = make(leaf=0.25)
    try:
        dev_add(m, pts, [100, 300, 300, 650])
        model.add(pts[100:650], [0, 200, 200, 550])
        check(m, model)
    finally:
        m.close()


def test_more_clouds_than_one_launch_takes_with_their_own_poses():
    """300 clouds: the offsets of 256 travel with a launch, so the call is two launches, and the second starts at pose 256"""
    rng = np.random.default_rng(41)
    sizes = np.resize([3, 0, 1, 7, 2, 0, 5], 300)
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    pts, _ = M.random_rays(41, int(offsets[-1]), 4.0)
    poses = np.stack([small_pose(rng, angle=0.8, shift=3.0) for _ in sizes])
    results = []
    for plain in (0, 1):
        m, model = make(leaf=0.25)
        try:
            with option("NO_OCCUPANCY_COMBINE", plain):
                dev_add(m, pts, offsets, poses)
            model.add(pts, offsets, poses)
            results.append(check(m, model, plain))
            assert m.claims() == (model.plain_claims if plain else model.wave_claims)  # (the model counts wavefronts per launch)
        finally:
            m.close()
    assert M.same_bytes(results[0][0], results[1][0])


def test_two_adds_equal_one_add_of_both_and_a_cleared_map_is_a_fresh_one():
    xyz, offsets, poses = clouds(33)
    cut = 6  # clouds of the first call
    params = dict(leaf=0.25, max_range=5.0, clip_long=0)
    m, model = make(**params)
    whole, _ = make(**params)
    try:
        dev_add(m, xyz, offsets[:cut + 1], poses[:cut])
        dev_add(m, xyz, offsets[cut:], poses[cut:])
        dev_add(whole, xyz, offsets, poses)
        model.add(xyz, offsets, poses)
        a, b = check(m, model, "two calls"), check(whole, model, "one call")
        assert M.same_bytes(a[0], b[0]) and m.stats().tobytes() == whole.stats().tobytes()
        m.clear()
        M.assert_stats_equal(m.stats(), M.OccupancyModel().stats(), "cleared")
        vmin, dims = model.bounds()
        counts, state = dev_box(m, vmin, dims)
        assert not counts.any() and not state.any() and m.claims() == 0
        m.add_cloud(xyz[offsets[9]:offsets[10]], poses[9])  # refill, through the host form
        model.clear()
        model.add(xyz[offsets[9]:offsets[10]], poses=poses[9:10])
        check(m, model, "refilled")
    finally:
        m.close(), whole.close()


def test_the_host_forms_equal_the_device_forms():
    pts, pose = M.random_rays(34, 1500, 6.0)
    wide = np.concatenate([pts, np.ones((len(pts), 1))], axis=1)
    m, model = make(leaf=0.25)
    try:
        m.add_cloud(wide, pose)
        m.add_cloud(pts[:300].astype(np.float32))
        m.add_cloud(np.empty((0, 3)))
        model.add(wide, poses=pose[None])
        model.add(pts[:300].astype(np.float32))
        check(m, model)
        vmin, dims = model.bounds()
        want = model.box(vmin, dims)
        counts, state = m.box(vmin, dims)
        assert M.same_bytes(counts, want[0]) and M.same_bytes(state, want[1])
        assert M.same_bytes(m.slice(vmin, dims), model.slice(vmin, dims))
        q = CM.pose_act(pose, pts[:200])
        got, want = m.query(np.concatenate([q, np.zeros((200, 2))], axis=1)), model.query(q)
        assert M.same_bytes(got[0], want[0]) and M.same_bytes(got[1], want[1]) and (got[1] == capi.OCC_OCCUPIED).sum() > 100
        with pytest.raises(ValueError):
            m.add_cloud(np.zeros((5, 2)))
        with pytest.raises(ValueError):
            m.add_cloud(pts, pose[:6])
    finally:
        m.close()


def test_a_map_too_small_says_so_and_works_again_after_clear():
    pts, _ = M.random_rays(35, 300, 6.0)
    m, _ = make(max_voxels=8, leaf=0.25)
    try:
        for plain in (0, 1):
            with option("NO_OCCUPANCY_COMBINE", plain):
                dev_add(m, pts)
            st = m.stats()
            assert int(st["overflow"]) > 0 and int(st["voxels"]) <= 16 and int(st["rays_offered"]) == 300 * (plain + 1)
        m.clear()
        model = M.OccupancyModel(leaf=0.25)
        near = np.array([[0.6, 0.1, 0.1], [0.1, 0.7, 0.1]])
        dev_add(m, near)
        model.add(near)
        check(m, model, "after clear")
    finally:
        m.close()


# ---- 4. the thresholds of a voxel's state --------------------------------------------------------------------------------------
@pytest.mark.parametrize("thresholds", [dict(min_hits=2, occ_ratio=0.0, min_passes=3), dict(min_hits=1, occ_ratio=0.5, min_passes=1),
                                        dict(min_hits=0, occ_ratio=0.0, min_passes=0)])
def test_states_under_other_thresholds(thresholds):
    pts, pose = M.random_rays(36, 2000, 4.0)
    m, model = make(leaf=0.25, **thresholds)
    try:
        dev_add(m, pts, poses=pose[None])
        model.add(pts, poses=pose[None])
        _, state = check(m, model, thresholds)
        if thresholds["min_hits"]:
            assert all((state == s).any() for s in (M.UNKNOWN, M.FREE, M.OCCUPIED))
        else:
            assert (state == M.OCCUPIED).all()  # (0 hits >= 0: every voxel, a voxel without a slot included)
    finally:
        m.close()


# ---- 5. read-outs --------------------------------------------------------------------------------------------------------------
def test_boxes_slices_and_optional_outputs():
    pts, pose = M.random_rays(37, 1500, 5.0)
    pose[4:] = [-3.3, 2.2, -0.9]
    m, model = make(leaf=0.25)
    try:
        dev_add(m, pts, poses=pose[None])
        model.add(pts, poses=pose[None])
        lo, dims = model.bounds()
        assert (lo < 0).all()
        sensor = np.floor(pose[4:] / 0.25).astype(np.int32)
        for vmin, d in ((lo, dims), (sensor, [1, 1, 1]), (lo, [dims[0], 1, 1]), (lo, [1, dims[1], 1]), ([sensor[0], sensor[1], lo[2]], [1, 1, dims[2]]),
                        (lo - 7, [3, 3, 3]), (sensor - 2, [5, 4, 3])):
            vmin, d = np.asarray(vmin, dtype=np.int32), np.asarray(d, dtype=np.uint32)
            want = model.box(vmin, d)
            got = dev_box(m, vmin, d)
            assert M.same_bytes(got[0], want[0]) and M.same_bytes(got[1], want[1]), (vmin, d)
            assert M.same_bytes(dev_box(m, vmin, d, with_state=False)[0], want[0]) and M.same_bytes(dev_box(m, vmin, d, with_counts=False)[1], want[1])
            assert dev_box(m, vmin, d, with_counts=False, with_state=False) == (None, None)
            grid = dev_slice(m, vmin, d)
            assert M.same_bytes(grid, model.slice(vmin, d)), (vmin, d)
        # a slice with columns nothing was seen in, and one level of it
        vmin, d = lo - [4, 4, 0], dims + [8, 8, 0]
        grid = dev_slice(m, vmin, d)
        assert M.same_bytes(grid, model.slice(vmin, d)) and (grid[:3] == M.UNKNOWN).all() and (grid[:, -3:] == M.UNKNOWN).all()
        assert all((grid == s).any() for s in (M.UNKNOWN, M.FREE, M.OCCUPIED))
        level = np.array([vmin[0], vmin[1], sensor[2]], dtype=np.int32)
        assert M.same_bytes(dev_slice(m, level, [d[0], d[1], 1]), model.slice(level, [d[0], d[1], 1]))
        assert not dev_slice(m, level, [d[0], d[1], 0]).any()  # no levels: every column unknown
        # voxels outside |v| < 2^20 read as unknown
        edge = np.array([M.BIAS - 2, 0, -M.BIAS - 1], dtype=np.int32)
        counts, state = dev_box(m, edge, [4, 1, 3])
        assert not counts.any() and not state.any()
        # query: optional outputs, a stride of 5
        q = CM.pose_act(pose, pts[:300])
        want = model.query(q)
        assert M.same_bytes(dev_query(m, q, with_state=False)[0], want[0]) and M.same_bytes(dev_query(m, q, with_counts=False)[1], want[1])
        wide = np.concatenate([q, np.full((300, 2), np.nan)], axis=1)
        got = dev_query(m, wide, stride=5)
        assert M.same_bytes(got[0], want[0]) and M.same_bytes(got[1], want[1])
        M.assert_stats_equal(m.stats(), model.stats(), "read-outs change nothing")
    finally:
        m.close()


def test_a_query_with_the_cloud_maps_centroids_finds_the_cloud_maps_counts():
    """both maps take the same call at equal leaf and equal ranges: a point the cloud map uses is a ray that hits, in the same voxel"""
    xyz, offsets, poses = clouds(38)
    c = ctx()
    leaf, lo, hi = 0.25, 0.5, 5.0
    m, model = make(leaf=leaf, min_range=lo, max_range=hi)
    cm = c.cloud_map(capi.CloudMapParams(leaf, lo, hi), 1 << 14)
    d_pts, d_poses = c.alloc(xyz.nbytes).upload(xyz), c.alloc(poses.nbytes).upload(poses)
    cap = 1 << 14
    bufs = [c.alloc(cap * 24), c.alloc(cap * 4), c.alloc(16), _poisoned(c, cap * 8), _poisoned(c, cap)]
    try:
        cm.add_clouds_dev(d_pts.ptr, 3, offsets, d_poses.ptr)
        m.add_clouds_dev(d_pts.ptr, 3, offsets, d_poses.ptr)  # side by side on the same buffers
        cm.emit_dev(bufs[0].ptr, cap, bufs[2].ptr, 1, bufs[1].ptr)
        m.query_dev(bufs[0].ptr, 3, cap, bufs[3].ptr, bufs[4].ptr)  # (the tail of the buffer is not centroids: only the first n are looked at)
        c.synchronize()
        n = int(bufs[2].download(np.uint32, 1)[0])
        assert 500 < n < cap
        count = bufs[1].download(np.uint32, cap)[:n]
        counts, state = bufs[3].download(np.uint32, cap * 2).reshape(-1, 2)[:n], bufs[4].download(np.uint8, cap)[:n]
        assert M.same_bytes(counts[:, 0], count) and (state == M.OCCUPIED).all()
        model.add(xyz, offsets, poses)
        centroids = bufs[0].download(np.float64, cap * 3).reshape(-1, 3)[:n]
        assert M.same_bytes(counts, model.query(centroids)[0])
        assert int(cm.stats()["points_used"]) == int(m.stats()["rays_hit"]) == int(count.sum())
    finally:
        for b in bufs + [d_pts, d_poses]:
            b.free()
        m.close(), cm.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def status_of(fn, *args, **kw):
    try:
        fn(*args, **kw)
        return capi.OK
    except capi.LoamxError as e:
        return e.status


def test_refusals_leave_the_map_as_it_was():
    c = ctx()
    nan, inf = float("nan"), float("inf")

    def create(max_voxels=64, **kw):
        def go():
            c.occupancy_map(capi.OccupancyParams(**kw), max_voxels).close()
        return status_of(go)

    assert create() == capi.OK and create(min_range=0.0, max_range=0.0, end_margin=0.0) == capi.OK and create(leaf=0.02, max_range=81.92) == capi.OK
    for kw in (dict(leaf=0.0), dict(leaf=-1.0), dict(leaf=nan), dict(leaf=inf), dict(min_range=-0.1), dict(min_range=nan), dict(min_range=inf),
               dict(max_range=0.4), dict(max_range=nan), dict(max_range=inf), dict(end_margin=-0.1), dict(end_margin=nan), dict(end_margin=inf),
               dict(occ_ratio=-0.5), dict(occ_ratio=nan), dict(occ_ratio=inf), dict(max_voxels=0)):
        assert create(**kw) == capi.ERR_BAD_PARAM, kw
    assert create(leaf=0.01, max_range=41.0) == capi.ERR_UNSUPPORTED and create(leaf=0.02, max_range=82.0) == capi.ERR_UNSUPPORTED
    assert create(max_voxels=(1 << 30) + 1) == capi.ERR_UNSUPPORTED
    lib, szp = c.lib, C.POINTER(C.c_size_t)
    st = capi.OccupancyParams().struct()
    h = C.c_void_p()
    assert lib.loamx_occupancy_create(c.h, None, 64, C.byref(h)) == capi.ERR_BAD_PARAM
    assert lib.loamx_occupancy_create(c.h, C.byref(st), 64, None) == capi.ERR_BAD_PARAM
    assert lib.loamx_occupancy_create(None, C.byref(st), 64, C.byref(h)) == capi.ERR_BAD_PARAM

    pts, _ = M.random_rays(39, 500, 5.0)
    m, model = make(leaf=0.25)
    d_pts, d_out = c.alloc(pts.nbytes).upload(pts), _poisoned(c, 4096)
    i32p, u32p = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
    try:
        dev_add(m, pts)
        model.add(pts)
        check(m, model)
        vmin, dims = model.bounds()
        before = snapshot(m, vmin, dims)
        one = np.array([0, 500], dtype=np.uint64)
        assert status_of(m.add_clouds_dev, d_pts.ptr, 2, one) == capi.ERR_BAD_PARAM                  # point_stride < 3
        assert status_of(m.add_clouds_dev, d_pts.ptr, 3, [0, 300, 200, 500]) == capi.ERR_BAD_PARAM  # descending offsets
        assert status_of(m.add_clouds_dev, 0, 3, one) == capi.ERR_BAD_PARAM                           # null points
        assert status_of(m.add_clouds_dev, d_pts.ptr, 1 << 32, one) == capi.ERR_UNSUPPORTED
        assert lib.loamx_occupancy_add_clouds_dev(c.h, m.h, d_pts.ptr, 3, None, 1, None) == capi.ERR_BAD_PARAM  # null offsets
        assert lib.loamx_occupancy_add_clouds_dev(c.h, None, d_pts.ptr, 3, one.ctypes.data_as(szp), 1, None) == capi.ERR_BAD_PARAM
        assert lib.loamx_occupancy_add_cloud(c.h, m.h, None, 3, 5, None) == capi.ERR_BAD_PARAM
        # the 2^32 - 2 total: in one call, and together with what the map already took (the call is refused before anything is read)
        assert status_of(m.add_clouds_dev, d_pts.ptr, 3, [0, (1 << 32) - 1]) == capi.ERR_UNSUPPORTED
        assert status_of(m.add_clouds_dev, d_pts.ptr, 3, [0, (1 << 32) - 2 - 499]) == capi.ERR_UNSUPPORTED
        assert status_of(m.query_dev, d_pts.ptr, 2, 10, d_out.ptr, d_out.ptr) == capi.ERR_BAD_PARAM
        assert status_of(m.query_dev, 0, 3, 10, d_out.ptr, d_out.ptr) == capi.ERR_BAD_PARAM
        assert status_of(m.query_dev, d_pts.ptr, 3, (1 << 31) + 1, d_out.ptr, d_out.ptr) == capi.ERR_UNSUPPORTED
        assert status_of(m.box_dev, vmin, [1 << 11, 1 << 11, (1 << 9) + 1], d_out.ptr, d_out.ptr) == capi.ERR_UNSUPPORTED
        assert status_of(m.slice_dev, vmin, [1 << 16, (1 << 15) + 1, 1], d_out.ptr) == capi.ERR_UNSUPPORTED
        assert status_of(m.slice_dev, vmin, [4, 4, 1], 0) == capi.ERR_BAD_PARAM
        v3, d3 = (C.c_int32 * 3)(0, 0, 0), (C.c_uint32 * 3)(2, 2, 2)
        assert lib.loamx_occupancy_box_dev(c.h, m.h, None, d3, d_out.ptr, d_out.ptr) == capi.ERR_BAD_PARAM
        assert lib.loamx_occupancy_box_dev(c.h, m.h, v3, None, d_out.ptr, d_out.ptr) == capi.ERR_BAD_PARAM
        assert lib.loamx_occupancy_box_dev(c.h, None, v3, d3, d_out.ptr, d_out.ptr) == capi.ERR_BAD_PARAM
        assert lib.loamx_occupancy_slice_dev(c.h, m.h, None, d3, d_out.ptr) == capi.ERR_BAD_PARAM
        assert lib.loamx_occupancy_stats_read(c.h, m.h, None) == capi.ERR_BAD_PARAM
        assert lib.loamx_occupancy_claims_read(c.h, m.h, None) == capi.ERR_BAD_PARAM
        assert lib.loamx_occupancy_clear(c.h, None) == capi.ERR_BAD_PARAM
        for bad in (([0, 0], [1, 1, 1]), ([0, 0, 0], [1, -1, 1]), ([0.5, 0, 0], [1, 1, 1]), ([1 << 31, 0, 0], [1, 1, 1])):
            with pytest.raises(ValueError):
                m.box_dev(bad[0], bad[1], d_out.ptr, d_out.ptr)
        with pytest.raises(ValueError):
            m.add_clouds_dev(d_pts.ptr, 3, [0, -5])
        c.synchronize()
        assert (d_out.download(np.uint8, 4096) == POISON).all()  # a refused call writes nothing
        after = snapshot(m, vmin, dims)
        assert M.same_bytes(after[0], before[0]) and M.same_bytes(after[1], before[1]) and after[2:] == before[2:]
        # nothing to do is not a refusal
        assert status_of(m.add_clouds_dev, d_pts.ptr, 3, [0, 0]) == capi.OK and status_of(m.add_clouds_dev, 0, 3, [7]) == capi.OK
        assert status_of(m.query_dev, 0, 3, 0, d_out.ptr, d_out.ptr) == capi.OK and status_of(m.box_dev, vmin, [3, 0, 3], d_out.ptr, d_out.ptr) == capi.OK
        assert status_of(m.slice_dev, vmin, [0, 5, 2], 0) == capi.OK
        c.synchronize()
        assert (d_out.download(np.uint8, 4096) == POISON).all()
        M.assert_stats_equal(m.stats(), model.stats(), "after the empty calls")
    finally:
        d_pts.free(), d_out.free(), m.close()
    with pytest.raises(ValueError):
        m.clear()  # closed


def test_a_map_belongs_to_the_context_that_created_it():
    m, model = make(leaf=0.25)
    other = capi.Context(0)
    d_out = other.alloc(64)
    try:
        pts, _ = M.random_rays(40, 200, 4.0)
        dev_add(m, pts)
        model.add(pts)
        lib = other.lib
        off = np.array([0, 1], dtype=np.uint64)
        v3, d3 = (C.c_int32 * 3)(0, 0, 0), (C.c_uint32 * 3)(1, 1, 1)
        assert lib.loamx_occupancy_clear(other.h, m.h) == capi.ERR_BAD_PARAM
        assert lib.loamx_occupancy_add_clouds_dev(other.h, m.h, d_out.ptr, 3, off.ctypes.data_as(C.POINTER(C.c_size_t)), 1, None) == capi.ERR_BAD_PARAM
        assert lib.loamx_occupancy_query_dev(other.h, m.h, d_out.ptr, 3, 1, d_out.ptr, None) == capi.ERR_BAD_PARAM
        assert lib.loamx_occupancy_box_dev(other.h, m.h, v3, d3, d_out.ptr, None) == capi.ERR_BAD_PARAM
        assert lib.loamx_occupancy_slice_dev(other.h, m.h, v3, d3, d_out.ptr) == capi.ERR_BAD_PARAM
        st = np.zeros(1, dtype=capi.OCCUPANCY_STATS_DTYPE)
        assert lib.loamx_occupancy_stats_read(other.h, m.h, st.ctypes.data) == capi.ERR_BAD_PARAM
        n = C.c_uint64(0)
        assert lib.loamx_occupancy_claims_read(other.h, m.h, C.byref(n)) == capi.ERR_BAD_PARAM
        check(m, model, "after the other context's calls")
    finally:
        d_out.free(), other.close(), m.close()


# ---- 7. an organised scan ----------------------------------------------------------------------------------------------------
def _free_then_wall_then_unknown(grid, sx, sy):
    """along the four grid directions from the sensor's cell: FREE cells in front of the first OCCUPIED cell and UNKNOWN cells behind it"""
    found = 0
    for line in (grid[sy, sx:], grid[sy, sx::-1], grid[sy:, sx], grid[sy::-1, sx]):
        occ = np.flatnonzero(line == M.OCCUPIED)
        if len(occ) and occ[0] > 2:
            k = occ[0]
            found += bool((line[1:k] == M.FREE).sum() >= 2 and (line[k + 1:] == M.UNKNOWN).any())
    return found


def test_an_organised_lot_scan_at_a_pose_of_a_composed_trajectory_and_its_slice_at_sensor_height():
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
    bufs = [c.alloc(cloud.nbytes).upload(cloud), c.alloc(H * W * 24), c.alloc(results.nbytes).upload(results), c.alloc(3 * 56)]
    d_cloud, d_scan, d_results, d_traj = bufs
    leaf = 0.4
    m, model = make(max_voxels=1 << 18, leaf=leaf, max_range=40.0)
    try:
        c.organize_clouds_dev(lay, d_cloud.ptr, 3, [0, H * W], d_scan.ptr)
        c.compose_trajectory_dev(d_results.ptr, 2, d_traj.ptr, origin=S.yaw_pose(yaw, origin))
        m.add_clouds_dev(d_scan.ptr, 3, [0, H * W], d_traj.ptr + 2 * 56)  # no host copy and no synchronise in between
        c.synchronize()
        organised = d_scan.download(np.float64, H * W * 3).reshape(-1, 3)
        traj = d_traj.download(np.float64, 21).reshape(3, 7)
        model.add(organised, poses=traj[2:3])
        st = model.stats()
        assert st["rays_hit"] > 1000 and st["visits"] > 20 * st["rays_hit"] and st["range_short"] > 0
        check(m, model)
        lo, dims = model.bounds()
        sensor = np.floor(traj[2, 4:] / leaf).astype(np.int64)
        vmin, d = np.array([lo[0], lo[1], sensor[2] - 1], dtype=np.int32), np.array([dims[0], dims[1], 3], dtype=np.uint32)
        want = model.slice(vmin, d)
        sx, sy = int(sensor[0] - lo[0]), int(sensor[1] - lo[1])
        assert want[sy, sx] == M.FREE and _free_then_wall_then_unknown(want, sx, sy) >= 1  # the scene first ...
        got = dev_slice(m, vmin, d)
        assert M.same_bytes(got, want) and _free_then_wall_then_unknown(got, sx, sy) >= 1  # ... then the kernel
    finally:
        for b in bufs:
            b.free()
        m.close(), lay.close()
