"""GPU: the cloud map (include/loamx.h, "cloud map"; loam_amd/csrc/cloudmap_kernels.hip) against the numpy model of
tests/cloudmap_common.py, by equality of bytes: centroids, counts, `first`, the voxel order, n_out and the stats. Outputs are
poisoned before every emit. Run combining and the plain one-point-one-claim form (context option NO_CLOUDMAP_COMBINE) must
agree with each other as well as with the model."""
import ctypes as C

import numpy as np
import pytest

import cloudmap_common as M
import outdoor_scenes as S
from gpu_common import ctx, option
from loam_amd import capi
from map_common import small_pose

pytestmark = pytest.mark.gpu

POISON = 0xA5
POISON_U32 = np.uint32(0xA5A5A5A5)
POISON_F64 = np.frombuffer(bytes([POISON] * 8), dtype=np.float64)[0]


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


def dev_emit(m, min_points=1, capacity=None, with_count=True, with_first=True):
    """emit_dev into poisoned buffers; returns (xyz, count, first, n) cut to min(n, capacity) after checking that nothing
    beyond was written (count / first are None where the output was not asked for)"""
    c = m.ctx
    capacity = m.max_voxels if capacity is None else capacity
    room = capacity + 3  # (what lies past the capacity must stay poison too)
    bufs = [c.alloc(room * 24), c.alloc(room * 4), c.alloc(room * 4), c.alloc(16)]
    try:
        for b in bufs:
            b.upload(np.full(b.nbytes, POISON, dtype=np.uint8))
        m.emit_dev(bufs[0].ptr, capacity, bufs[3].ptr, min_points, bufs[1].ptr if with_count else 0, bufs[2].ptr if with_first else 0)
        c.synchronize()
        xyz = bufs[0].download(np.float64, room * 3).reshape(room, 3)
        count, first = bufs[1].download(np.uint32, room), bufs[2].download(np.uint32, room)
        n_words = bufs[3].download(np.uint32, 4)
    finally:
        for b in bufs:
            b.free()
    n = int(n_words[0])
    assert (n_words[1:] == POISON_U32).all()
    k = min(n, capacity)
    assert (xyz[k:].view(np.uint64) == POISON_F64.view(np.uint64)).all(), "centroids written past min(n, capacity)"
    assert (count[k if with_count else 0:] == POISON_U32).all() and (first[k if with_first else 0:] == POISON_U32).all()
    return xyz[:k].copy(), count[:k].copy() if with_count else None, first[:k].copy() if with_first else None, n


def check(m, model, what="", min_points=1):
    got = dev_emit(m, min_points)
    M.assert_emit_equal(got, model.emit(min_points), what)
    M.assert_stats_equal(m.stats(), model.stats(), what)
    return got


def make(leaf=0.5, min_range=0.5, max_range=120.0, max_voxels=4096):
    return ctx().cloud_map(capi.CloudMapParams(leaf, min_range, max_range), max_voxels), M.CloudMapModel(leaf, min_range, max_range)


# ---- 1. cloud sizes ----------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 63, 64, 0, 65, 255, 256, 257, 1000, 0)  # an empty cloud first, in the middle and last


@pytest.mark.parametrize("dtype,stride", [(np.float64, 3), (np.float64, 5), (np.float32, 3), (np.float32, 5)])
def test_clouds_of_every_size_in_one_batch_with_their_own_device_poses(dtype, stride):
    rng = np.random.default_rng(21)
    n = sum(SIZES)
    pts = np.full((n, stride), np.nan)  # (the scalars behind z are never read)
    pts[:, :3] = rng.uniform(-3, 3, (n, 3)) * [1.0, 1.0, 0.2]
    pts = pts.astype(dtype)
    offsets = np.concatenate([[0], np.cumsum(SIZES)])
    poses = np.stack([small_pose(rng, angle=0.3, shift=2.0) for _ in SIZES])
    m, model = make()
    try:
        dev_add(m, pts, offsets, poses)
        model.add(pts, offsets, poses)
        got = check(m, model)
        assert got[3] > 200 and got[1].max() > 2  # (shared voxels and plenty of them)
    finally:
        m.close()


def test_offsets_that_do_not_start_at_zero_count_from_the_first_offset():
    rng = np.random.default_rng(22)
    pts = rng.uniform(-4, 4, (700, 3))
    m, model = make()
    try:
        dev_add(m, pts, [100, 300, 300, 650])
        model.add(pts[100:650], [0, 200, 200, 550])
        check(m, model)
    finally:
        m.close()


# ---- 2. runs -----------------------------------------------------------------------------------------------------------------
def _own(i):
    """a point alone in voxel number i (leaf 1)"""
    i = np.asarray(i)
    return np.stack([(i % 64) + 0.5, (i // 64) + 0.25, np.full(i.shape, 3.75)], axis=-1)


def _in_voxel(rng, n, corner):
    return np.asarray(corner, dtype=np.float64) + rng.uniform(0.0, 1.0, (n, 3))


def run_patterns():
    rng = np.random.default_rng(23)
    out = {}
    out["one_voxel"] = _in_voxel(rng, 4096, (5, 5, 0))
    out["all_alone"] = _own(np.arange(1000))
    ab = np.where((np.arange(300) % 2 == 0)[:, None], _in_voxel(rng, 300, (2, 0, 0)), _in_voxel(rng, 300, (-3, 1, 0)))
    out["a_b_a_b"] = ab
    for name, lo, hi, n in (("lane_63_64", 60, 71, 200), ("thread_255_256", 250, 263, 600)):
        p = _own(np.arange(n))
        p[lo:hi] = _in_voxel(rng, hi - lo, (-7, -7, 1))
        out[name] = p
    p = _own(np.arange(200))
    p[10:21] = _in_voxel(rng, 11, (-7, -7, 1))
    p[15] = [np.nan, 0.0, 0.0]
    p[100:111] = _in_voxel(rng, 11, (-9, 4, 1))
    p[104] = [0.0, 0.0, 0.0]
    out["interrupted"] = p
    return out


PATTERNS = run_patterns()


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_runs_inside_and_across_wavefronts_combined_and_plain(name):
    pts = PATTERNS[name]
    results = []
    for plain in (0, 1):
        m, model = make(leaf=1.0, min_range=0.1)
        try:
            with option("NO_CLOUDMAP_COMBINE", plain):
                dev_add(m, pts)
            model.add(pts)
            results.append(check(m, model, (name, plain)))
            # the claims: one per used point in the plain form, one per run of a wavefront with combining (A B A: three)
            ok = M.validity(pts, 0.1, 120.0) == M.USED
            cell_ok, v, _ = M.cells(pts, 1.0)
            assert m.claims() == (int((ok & cell_ok).sum()) if plain else M.wave_runs(ok & cell_ok, M.pack(v))), (name, plain)
        finally:
            m.close()
    M.assert_emit_equal(results[0], results[1], name)
    n_vox = {"one_voxel": 1, "all_alone": 1000, "a_b_a_b": 2, "lane_63_64": 190, "thread_255_256": 588, "interrupted": 180}[name]
    assert results[0][3] == n_vox
    if name == "interrupted":
        assert results[0][1][10] == 10 and results[0][2][10] == 10  # the voxel of the run with the NaN in it: ten points, first one 10


def test_a_point_out_of_voxel_range_behind_a_run_leaves_nothing_in_the_runs_sums():
    """A point whose voxel is out of range on ONE axis has offsets on the other two. It sits in the lanes behind a run and
    carries that run's number, so whatever it held would reach the run's head: it must hold zeros. (NaN, Inf and
    range-dropped points never get as far as an offset, so they cannot show this.)"""
    leaf = 1e-4  # voxels reach to +-104.86 m, max_range 120 m lets a point at x = 110 m through to the voxel step
    a = np.array([[1.03005, 1.03005, 1.03005], [1.03007, 1.03006, 1.03008]])              # one voxel
    b = np.array([[2.00011, 2.00012, 2.00013], [2.00015, 2.00017, 2.00019], [2.00012, 2.00018, 2.00016]])  # another
    x = np.array([[110.000037, 1.070053, 1.090071], [1.050041, -108.000029, 1.030067], [1.010013, 1.020059, 111.000083]])
    t = x / leaf
    frac = t - np.floor(t)
    assert (np.floor(frac * M.UNIT) > 0).all() and (np.abs(np.floor(t)) >= M.BIAS).sum(axis=1).tolist() == [1, 1, 1]
    filler = _own(np.arange(40))
    cases = {
        "behind_a_run": np.concatenate([a, x[:1]]),
        "three_behind_a_run": np.concatenate([b, x]),
        "inside_a_voxels_points": np.concatenate([a[:1], a[1:], x[1:2], a[::-1]]),
        "in_front_and_behind": np.concatenate([x[2:], a, x[:2], b, x]),
        "across_lane_63_64": np.concatenate([filler, filler[:22] + [0.0, 70.0, 0.0], b[:2], x, b[2:], a, x[:1]]),
    }
    for name, pts in cases.items():
        results = []
        for plain in (0, 1):
            m, model = make(leaf=leaf, min_range=0.1, max_range=120.0)
            try:
                with option("NO_CLOUDMAP_COMBINE", plain):
                    dev_add(m, pts)
                model.add(pts)
                results.append(check(m, model, (name, plain)))
                assert int(m.stats()["outside"]) == int((np.abs(pts) > 100).any(axis=1).sum()) > 0
            finally:
                m.close()
        M.assert_emit_equal(results[0], results[1], name)


# ---- 3. dropped points -------------------------------------------------------------------------------------------------------
def test_every_kind_of_dropped_point_is_counted_in_its_own_word_and_keeps_its_index():
    lo, hi = 0.5, 40.0
    a = np.array([[0, 0, 0], [1, 1, 1], [np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [0, 0, 0],
                  [lo, 0, 0], [np.nextafter(lo, 0), 0, 0], [0, np.nextafter(lo, 1), 0],
                  [0, 0, hi], [0, 0, np.nextafter(hi, np.inf)], [np.nextafter(hi, 0), 0, 0], [1e200, 0, 0], [2, 2, 2]], dtype=np.float64)
    b = np.array([[1, 2, 3], [0, 0, 0], [3, 2, 1]], dtype=np.float64)   # at a pose that carries them out of the voxel range
    pts, offsets = np.concatenate([a, b, a]), [0, len(a), len(a) + len(b), 2 * len(a) + len(b)]
    poses = np.array([[0, 0, 0, 1.0, 0, 0, 0], [0, 0, 0, 1.0, 3e5, 0, 0], [0, 0, 0, 1.0, 0.25, 0, 0]])
    m, model = make(leaf=0.2, min_range=lo, max_range=hi)
    try:
        dev_add(m, pts, offsets, poses)
        model.add(pts, offsets, poses)
        got = check(m, model)
        st = m.stats()
        assert (int(st["invalid"]), int(st["range"]), int(st["outside"]), int(st["points_used"])) == (8, 9, 2, 12)
        assert int(st["points_offered"]) == len(pts) and got[2].tolist() == [1, 6, 8, 9, 11, 13, 18, 23, 25, 26, 28, 30]
    finally:
        m.close()


# ---- 4. two adds, clear, determinism -----------------------------------------------------------------------------------------
def test_two_adds_list_voxels_by_first_appearance_and_a_cleared_map_is_a_fresh_one():
    rng = np.random.default_rng(24)
    first_call = rng.uniform(-5, 5, (3000, 3))
    second_call = np.concatenate([rng.uniform(-5, 5, (1500, 3)), rng.uniform(5, 9, (1500, 3))])[rng.permutation(3000)]
    pose2 = small_pose(rng, angle=0.05, shift=0.5)[None]

    def program(m):
        dev_add(m, first_call)
        first = dev_emit(m)
        dev_add(m, second_call, poses=pose2)
        return first, dev_emit(m), m.stats()

    m, model = make(leaf=0.5, max_voxels=1 << 15)
    other, _ = make(leaf=0.5, max_voxels=1 << 15)
    try:
        f1, e1, s1 = program(m)
        model.add(first_call)
        M.assert_emit_equal(f1, model.emit(), "first call")
        model.add(second_call, poses=pose2)
        M.assert_emit_equal(e1, model.emit(), "both calls")
        M.assert_stats_equal(s1, model.stats())
        n1 = f1[3]
        assert M.same_bytes(e1[2][:n1], f1[2]) and (e1[2][n1:] >= 3000).all() and e1[3] > n1  # old voxels keep their place, new ones follow
        assert (e1[1][:n1] >= f1[1]).all() and (e1[1][:n1] > f1[1]).any() and int(e1[1].sum()) == int(s1["points_used"])
        m.clear()
        M.assert_stats_equal(m.stats(), M.CloudMapModel().stats(), "cleared")
        assert dev_emit(m)[3] == 0
        f2, e2, s2 = program(m)  # the cleared map ...
        f3, e3, s3 = program(other)  # ... and a fresh one
        for a, b in ((f2, f1), (e2, e1), (f3, f1), (e3, e1)):
            M.assert_emit_equal(a, b)
        M.assert_stats_equal(s2, s1), M.assert_stats_equal(s3, s1)
    finally:
        m.close(), other.close()


# ---- 5. emit -----------------------------------------------------------------------------------------------------------------
def test_emit_by_min_points_capacity_and_optional_outputs():
    rng = np.random.default_rng(25)
    pts = rng.normal(size=(4000, 3)) * [3.0, 3.0, 0.5]
    m, model = make(leaf=0.5, min_range=0.0)
    try:
        dev_add(m, pts)
        model.add(pts)
        full = model.emit()
        assert full[1].max() >= 3 and (full[1] == 1).any()
        for min_points in (1, 2, int(full[1].max()) + 1):
            got = check(m, model, min_points, min_points=min_points)
            assert (got[3] == 0) == (min_points > full[1].max())
        for min_points in (1, 2):
            n = model.emit(min_points)[3]
            for capacity in (0, 1, n // 2, n - 1, n, n + 1):
                M.assert_emit_equal(dev_emit(m, min_points, capacity), model.emit(min_points, capacity), (min_points, capacity))
        want = model.emit(2, 100)
        for with_count, with_first in ((False, True), (True, False), (False, False)):
            xyz, count, first, n = dev_emit(m, 2, 100, with_count, with_first)
            assert n == want[3] and M.same_bytes(xyz, want[0])
            assert (count is None or M.same_bytes(count, want[1])) and (first is None or M.same_bytes(first, want[2]))
        M.assert_emit_equal(dev_emit(m), dev_emit(m))  # emit does not change the map
        M.assert_stats_equal(m.stats(), model.stats())
        # the host form
        xyz, count, first, n = m.emit(2, capacity=50)
        M.assert_emit_equal((xyz, count, first, n), model.emit(2, 50), "host emit")
        M.assert_emit_equal(m.emit(), full, "host emit, everything")
    finally:
        m.close()


def test_the_host_add_equals_the_device_add():
    rng = np.random.default_rng(26)
    pts, pose = rng.uniform(-5, 5, (1500, 4)), small_pose(rng, angle=0.2, shift=1.0)
    m, model = make()
    try:
        m.add_cloud(pts, pose)
        m.add_cloud(pts[:300].astype(np.float32))
        m.add_cloud(np.empty((0, 3)))
        model.add(pts, poses=pose[None])
        model.add(pts[:300].astype(np.float32))
        check(m, model)
        with pytest.raises(ValueError):
            m.add_cloud(np.zeros((5, 2)))
        with pytest.raises(ValueError):
            m.add_cloud(pts, pose[:6])
    finally:
        m.close()


# ---- 6. overflow -------------------------------------------------------------------------------------------------------------
def test_a_map_too_small_says_so_and_works_again_after_clear():
    pts = _own(np.arange(100))
    m, _ = make(leaf=1.0, min_range=0.1, max_voxels=8)
    try:
        for plain in (0, 1):
            with option("NO_CLOUDMAP_COMBINE", plain):
                dev_add(m, pts)
            st = m.stats()
            assert int(st["overflow"]) > 0 and int(st["voxels"]) <= 8 and int(st["points_offered"]) == 100 * (plain + 1)
            assert dev_emit(m)[3] <= 8
        m.clear()
        model = M.CloudMapModel(1.0, 0.1, 120.0)
        dev_add(m, pts[:8])
        model.add(pts[:8])
        check(m, model, "after clear")
    finally:
        m.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------
def status_of(fn, *args, **kw):
    try:
        fn(*args, **kw)
        return capi.OK
    except capi.LoamxError as e:
        return e.status


def test_refusals_leave_the_map_as_it_was():
    c = ctx()
    nan, inf = float("nan"), float("inf")

    def create(leaf=0.2, lo=0.5, hi=120.0, max_voxels=64):
        def go():
            c.cloud_map(capi.CloudMapParams(leaf, lo, hi), max_voxels).close()
        return status_of(go)

    assert create() == capi.OK and create(lo=0.0, hi=0.0) == capi.OK
    for kw in (dict(leaf=0.0), dict(leaf=-1.0), dict(leaf=nan), dict(leaf=inf), dict(lo=-0.1), dict(lo=nan), dict(lo=inf), dict(hi=0.4),
               dict(hi=nan), dict(max_voxels=0)):
        assert create(**kw) == capi.ERR_BAD_PARAM, kw
    assert create(max_voxels=(1 << 30) + 1) == capi.ERR_UNSUPPORTED
    lib, szp = c.lib, C.POINTER(C.c_size_t)
    st = capi.CloudMapParams().struct()
    h = C.c_void_p()
    assert lib.loamx_cloud_map_create(c.h, None, 64, C.byref(h)) == capi.ERR_BAD_PARAM
    assert lib.loamx_cloud_map_create(c.h, C.byref(st), 64, None) == capi.ERR_BAD_PARAM
    assert lib.loamx_cloud_map_create(None, C.byref(st), 64, C.byref(h)) == capi.ERR_BAD_PARAM

    rng = np.random.default_rng(27)
    pts = rng.uniform(-5, 5, (500, 3))
    m, model = make()
    d_pts, d_out = c.alloc(pts.nbytes).upload(pts), c.alloc(4096)
    try:
        dev_add(m, pts)
        model.add(pts)
        before = check(m, model)
        one = np.array([0, 500], dtype=np.uint64)
        assert status_of(m.add_clouds_dev, d_pts.ptr, 2, one) == capi.ERR_BAD_PARAM                  # point_stride < 3
        assert status_of(m.add_clouds_dev, d_pts.ptr, 3, [0, 300, 200, 500]) == capi.ERR_BAD_PARAM  # descending offsets
        assert status_of(m.add_clouds_dev, 0, 3, one) == capi.ERR_BAD_PARAM                           # null points
        assert lib.loamx_cloud_map_add_clouds_dev(c.h, m.h, d_pts.ptr, 3, None, 1, None) == capi.ERR_BAD_PARAM  # null offsets
        assert lib.loamx_cloud_map_add_clouds_dev(c.h, None, d_pts.ptr, 3, one.ctypes.data_as(szp), 1, None) == capi.ERR_BAD_PARAM
        assert lib.loamx_cloud_map_add_cloud(c.h, m.h, None, 3, 5, None) == capi.ERR_BAD_PARAM
        # the 2^32 - 2 total: in one call, and together with what the map already took (the call is refused before anything is read)
        assert status_of(m.add_clouds_dev, d_pts.ptr, 3, [0, (1 << 32) - 1]) == capi.ERR_UNSUPPORTED
        assert status_of(m.add_clouds_dev, d_pts.ptr, 3, [0, (1 << 32) - 2 - 499]) == capi.ERR_UNSUPPORTED
        with pytest.raises(ValueError):
            m.add_clouds_dev(d_pts.ptr, 3, [0, -5])
        with pytest.raises(ValueError):
            m.add_clouds_dev(d_pts.ptr, 3, np.array([0.0, 5.0]))
        assert status_of(m.emit_dev, d_out.ptr, 10, 0) == capi.ERR_BAD_PARAM    # null d_n_out
        assert status_of(m.emit_dev, 0, 10, d_out.ptr) == capi.ERR_BAD_PARAM    # null d_xyz_out with room asked for
        assert lib.loamx_cloud_map_stats_read(c.h, m.h, None) == capi.ERR_BAD_PARAM
        assert lib.loamx_cloud_map_clear(c.h, None) == capi.ERR_BAD_PARAM
        with pytest.raises(ValueError):
            m.emit_dev(d_out.ptr, -1, d_out.ptr)
        M.assert_emit_equal(dev_emit(m), before, "after the refusals")
        M.assert_stats_equal(m.stats(), model.stats(), "after the refusals")
        assert status_of(m.add_clouds_dev, d_pts.ptr, 3, [0, 0]) == capi.OK and status_of(m.add_clouds_dev, 0, 3, [7]) == capi.OK  # nothing to add
        M.assert_stats_equal(m.stats(), model.stats(), "after the empty calls")
    finally:
        d_pts.free(), d_out.free(), m.close()
    with pytest.raises(ValueError):
        m.clear()  # closed


def test_a_map_belongs_to_the_context_that_created_it():
    m, model = make()
    other = capi.Context(0)
    d_out = other.alloc(64)
    try:
        pts = np.random.default_rng(29).uniform(-3, 3, (200, 3))
        dev_add(m, pts)
        model.add(pts)
        lib = other.lib
        off = np.array([0, 1], dtype=np.uint64)
        assert lib.loamx_cloud_map_clear(other.h, m.h) == capi.ERR_BAD_PARAM
        assert lib.loamx_cloud_map_add_clouds_dev(other.h, m.h, d_out.ptr, 3, off.ctypes.data_as(C.POINTER(C.c_size_t)), 1, None) == capi.ERR_BAD_PARAM
        assert lib.loamx_cloud_map_emit_dev(other.h, m.h, 1, d_out.ptr, None, None, 1, d_out.ptr) == capi.ERR_BAD_PARAM
        st = np.zeros(1, dtype=capi.CLOUD_MAP_STATS_DTYPE)
        assert lib.loamx_cloud_map_stats_read(other.h, m.h, st.ctypes.data) == capi.ERR_BAD_PARAM
        check(m, model, "after the other context's calls")
    finally:
        d_out.free(), other.close(), m.close()


# ---- 8. an organised scan ----------------------------------------------------------------------------------------------------
def test_an_organised_scan_from_organize_and_deskew_at_a_pose_of_a_composed_trajectory():
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
    motion = S.yaw_pose(0.02, [0.3, 0.0, 0.0])
    bufs = [c.alloc(cloud.nbytes).upload(cloud), c.alloc(H * W * 24), c.alloc(results.nbytes).upload(results), c.alloc(3 * 56),
            c.alloc(56).upload(motion)]
    d_cloud, d_scan, d_results, d_traj, d_motion = bufs
    m, model = make(leaf=0.2)
    try:
        c.organize_clouds_dev(lay, d_cloud.ptr, 3, [0, H * W], d_scan.ptr)
        c.deskew_scans_dev(d_scan.ptr, 1, lidar, d_motion.ptr, d_scan.ptr, ref_fraction=1.0)
        c.compose_trajectory_dev(d_results.ptr, 2, d_traj.ptr, origin=S.yaw_pose(yaw, origin))
        m.add_clouds_dev(d_scan.ptr, 3, [0, H * W], d_traj.ptr + 2 * 56)  # no host copy and no synchronise in between
        c.synchronize()
        deskewed = d_scan.download(np.float64, H * W * 3).reshape(-1, 3)
        traj = d_traj.download(np.float64, 21).reshape(3, 7)
        model.add(deskewed, poses=traj[2:3])
        got = check(m, model)
        st = m.stats()
        assert int(st["range"]) > 0 and got[3] > 1000 and int(st["overflow"]) == 0
    finally:
        for b in bufs:
            b.free()
        m.close(), lay.close()
