"""GPU: the surfel map (include/loamx.h, "surfel map"; loam_amd/csrc/surfel_kernels.hip) against the Python model of
tests/surfel_common.py, by equality of bytes: the records (mean, covariance, eigenvalues, normal, count, first), the voxel order,
n_out, the stats, and the claims of the accumulate kernel against the model's. Outputs are poisoned before every read-out. Run
combining and the plain one-point-one-claim form (context option NO_SURFEL_COMBINE) must agree with each other as well as with
the model."""
import ctypes as C

import numpy as np
import pytest

import cloudmap_common as CM
import outdoor_scenes as S
import surfel_common as M
from gpu_common import ctx, option
from loam_amd import capi
from map_common import small_pose

pytestmark = pytest.mark.gpu

POISON = 0xA5
POISON_U32 = np.uint32(0xA5A5A5A5)
REC = M.SURFEL_DTYPE.itemsize


def test_the_layers_agree_on_the_record():
    assert capi.SURFEL_DTYPE == M.SURFEL_DTYPE and capi.SURFEL_DTYPE.itemsize == 128
    assert capi.SURFEL_MAP_STATS_DTYPE.names == M.STAT_NAMES
    p = capi.SurfelMapParams()
    assert (p.leaf, p.min_range, p.max_range) == M.DEFAULTS


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


def poisoned(c, nbytes):
    return c.alloc(nbytes).upload(np.full(nbytes, POISON, dtype=np.uint8))


def is_poison(a):
    return bool((np.ascontiguousarray(a).reshape(-1).view(np.uint8) == POISON).all())


def dev_emit(m, min_points=1, capacity=None, rec=True, xyz=True, normal=True):
    """emit_dev into poisoned buffers; (records, xyz, normal, n) cut to min(n, capacity) after checking that nothing beyond was
    written and that an output not asked for was not touched (it is None then)"""
    c = m.ctx
    capacity = m.max_voxels if capacity is None else capacity
    room = capacity + 3  # (what lies past the capacity must stay poison too)
    bufs = [poisoned(c, room * REC), poisoned(c, room * 24), poisoned(c, room * 24), poisoned(c, 16)]
    try:
        m.emit_dev(capacity, bufs[3].ptr, min_points, bufs[0].ptr if rec else 0, bufs[1].ptr if xyz else 0, bufs[2].ptr if normal else 0)
        c.synchronize()
        r = bufs[0].download(M.SURFEL_DTYPE, room)
        x, nn = bufs[1].download(np.float64, room * 3).reshape(room, 3), bufs[2].download(np.float64, room * 3).reshape(room, 3)
        n_words = bufs[3].download(np.uint32, 4)
    finally:
        for b in bufs:
            b.free()
    n = int(n_words[0])
    assert (n_words[1:] == POISON_U32).all()
    k = min(n, capacity)
    assert is_poison(r[k if rec else 0:]) and is_poison(x[k if xyz else 0:]) and is_poison(nn[k if normal else 0:]), "written past min(n, capacity)"
    return r[:k].copy() if rec else None, x[:k].copy() if xyz else None, nn[:k].copy() if normal else None, n


def check_emit(got, want, what=""):
    """got: dev_emit's; want: the model's (records, n)"""
    assert got[3] == want[1], (what, got[3], want[1])
    if got[0] is not None:
        M.assert_records_equal(got[0], want[0], what)
    if got[1] is not None:
        assert M.same_bytes(got[1], np.ascontiguousarray(want[0]["mean"])), (what, "means")
    if got[2] is not None:
        assert M.same_bytes(got[2], np.ascontiguousarray(want[0]["normal"])), (what, "normals")


def check(m, model, what="", min_points=1):
    got = dev_emit(m, min_points)
    check_emit(got, model.emit(min_points), what)
    M.assert_stats_equal(m.stats(), model.stats(), what)
    return got


def dev_query(m, pts, min_points=1, rec=True, dist=True, cnt=True, stride=None):
    c = m.ctx
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    n = len(pts)
    bufs = [c.alloc(max(pts.nbytes, 8)), poisoned(c, (n + 2) * REC), poisoned(c, (n + 2) * 8), poisoned(c, (n + 2) * 4)]
    try:
        if n:
            bufs[0].upload(pts)
        m.query_dev(bufs[0].ptr, stride or pts.shape[1], n, min_points, bufs[1].ptr if rec else 0, bufs[2].ptr if dist else 0, bufs[3].ptr if cnt else 0)
        c.synchronize()
        r, d, k = bufs[1].download(M.SURFEL_DTYPE, n + 2), bufs[2].download(np.float64, n + 2), bufs[3].download(np.uint32, n + 2)
    finally:
        for b in bufs:
            b.free()
    assert is_poison(r[n if rec else 0:]) and is_poison(d[n if dist else 0:]) and is_poison(k[n if cnt else 0:])
    return r[:n].copy() if rec else None, d[:n].copy() if dist else None, k[:n].copy() if cnt else None


def check_query(got, want, what=""):
    if got[0] is not None:
        M.assert_records_equal(got[0], want[0], what)
    if got[1] is not None:
        assert M.same_bytes(got[1], want[1]), (what, "distances")
    if got[2] is not None:
        assert M.same_bytes(got[2], want[2]), (what, "counts")


def make(leaf=0.5, min_range=0.5, max_range=120.0, max_voxels=4096):
    return ctx().surfel_map(capi.SurfelMapParams(leaf, min_range, max_range), max_voxels), M.SurfelMapModel(leaf, min_range, max_range)


def both_forms(pts, offsets=None, poses=None, what="", **kw):
    """the same call in both forms on fresh maps: bytes against the model and each other, claims against the model's"""
    results = []
    for plain in (0, 1):
        m, model = make(**kw)
        try:
            with option("NO_SURFEL_COMBINE", plain):
                dev_add(m, pts, offsets, poses)
            model.add(pts, offsets, poses)
            results.append(check(m, model, (what, plain)))
            assert m.claims() == (model.plain_claims if plain else model.wave_claims), (what, plain)
        finally:
            m.close()
    M.assert_records_equal(results[0][0], results[1][0], what)
    return results[0], model


# ---- 1. the shared cases ---------------------------------------------------------------------------------------------------------
CASES = M.shared_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_shared_case(name):
    leaf, pts, pose = CASES[name]
    got, model = both_forms(pts, poses=None if pose is None else pose[None], what=name, leaf=leaf, min_range=0.0)
    assert got[3] == len(model.vox) >= 1


def test_the_140000_point_voxel():
    leaf, pts = M.big_voxel()
    got, model = both_forms(pts, what="big voxel", leaf=leaf, min_range=0.0)
    (e,) = model.vox.values()
    assert got[3] == 1 and got[0]["count"][0] == 140000 and e[4] * e[2][0] >= 1 << 64
    assert model.wave_claims == (140000 + 63) // 64 and model.plain_claims == 140000


# ---- 2. cloud sizes, types, strides, poses -----------------------------------------------------------------------------------------
SIZES = (0, 1, 63, 64, 0, 65, 255, 256, 257, 1000, 0)  # an empty cloud first, in the middle and last


@pytest.mark.parametrize("dtype,stride,with_poses", [(np.float64, 3, True), (np.float64, 5, False), (np.float32, 3, False), (np.float32, 5, True)])
def test_clouds_of_every_size_in_one_batch(dtype, stride, with_poses):
    rng = np.random.default_rng(41)
    n = sum(SIZES)
    pts = np.full((n, stride), np.nan)  # (the scalars behind z are never read)
    pts[:, :3] = rng.uniform(-3, 3, (n, 3)) * [1.0, 1.0, 0.2]
    pts = pts.astype(dtype)
    offsets = np.concatenate([[0], np.cumsum(SIZES)])
    poses = np.stack([small_pose(rng, angle=0.3, shift=2.0) for _ in SIZES]) if with_poses else None
    got, _ = both_forms(pts, offsets, poses, what=(dtype, stride))
    assert got[3] > 100 and got[0]["count"].max() > 5


def test_offsets_that_do_not_start_at_zero_count_from_the_first_offset():
    rng = np.random.default_rng(42)
    pts = rng.uniform(-4, 4, (700, 3))
    m, model = make()
    try:
        dev_add(m, pts, [100, 300, 300, 650])
        model.add(pts[100:650], [0, 200, 200, 550])
        check(m, model)
    finally:
        m.close()


def test_more_than_256_clouds_in_one_call_are_two_launches():
    rng = np.random.default_rng(43)
    sizes = rng.integers(0, 9, 300)
    sizes[255:258] = (70, 0, 130)  # a run that would cross the boundary between the launches if the wavefronts did not restart there
    n = int(sizes.sum())
    pts = rng.uniform(-2, 2, (n, 3))
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    a = int(offsets[255])
    pts[a:a + 200] = [1.25, 1.25, 0.25] + rng.uniform(0, 0.2, (200, 3))
    poses = np.stack([small_pose(rng, angle=0.01, shift=0.01) for _ in sizes])
    poses[255:258] = [0, 0, 0, 1.0, 0, 0, 0]
    got, model = both_forms(pts, offsets, poses, what="300 clouds")
    assert model.wave_claims < model.plain_claims


def test_a_call_of_more_than_one_round_of_points():
    """kCloudChunkPoints + 1000 float points of a few voxels without poses: the second round of launches continues the running index"""
    n = M.CHUNK_POINTS + 1000
    rng = np.random.default_rng(44)
    pts = (rng.integers(0, 3, (n, 3)) + rng.random((n, 3))).astype(np.float32) + np.float32(1.0)
    m, model = make(leaf=1.0, max_voxels=256)
    try:
        dev_add(m, pts)
        model.add(pts)
        got = check(m, model)
        assert 27 <= got[3] <= 64 and int(got[0]["count"].astype(np.int64).sum()) == n
        assert m.claims() == model.wave_claims
    finally:
        m.close()


# ---- 3. runs -------------------------------------------------------------------------------------------------------------------------
def _own(i):
    """a point alone in voxel number i (leaf 1)"""
    i = np.asarray(i)
    return np.stack([(i % 64) + 0.5, (i // 64) + 0.25, np.full(i.shape, 3.75)], axis=-1)


def _in_voxel(rng, n, corner):
    return np.asarray(corner, dtype=np.float64) + rng.uniform(0.0, 1.0, (n, 3))


def run_patterns():
    rng = np.random.default_rng(45)
    out = {}
    out["one_run_of_64"] = np.concatenate([_own(np.arange(64)), _in_voxel(rng, 64, (5, 5, 0)), _own(np.arange(64, 70))])
    out["one_voxel"] = _in_voxel(rng, 4096, (5, 5, 0))
    out["all_alone"] = _own(np.arange(1000))
    out["a_b_a"] = np.concatenate([_in_voxel(rng, 5, (2, 0, 0)), _in_voxel(rng, 7, (-3, 1, 0)), _in_voxel(rng, 4, (2, 0, 0))])
    out["a_b_a_b"] = np.where((np.arange(300) % 2 == 0)[:, None], _in_voxel(rng, 300, (2, 0, 0)), _in_voxel(rng, 300, (-3, 1, 0)))
    for name, lo, hi, n in (("lane_63_64", 60, 71, 200), ("thread_255_256", 250, 263, 600)):
        p = _own(np.arange(n))
        p[lo:hi] = _in_voxel(rng, hi - lo, (-7, -7, 1))
        out[name] = p
    p = _own(np.arange(300))
    p[10:21] = _in_voxel(rng, 11, (-7, -7, 1))
    p[15] = [np.nan, 0.0, 0.0]            # invalid
    p[100:111] = _in_voxel(rng, 11, (-9, 4, 1))
    p[104] = [0.0, 0.0, 2.0]              # range (the test hands the points over 2 m lower, at a pose that lifts them again: the sensor's origin)
    p[200:211] = _in_voxel(rng, 11, (-9, 9, 1))
    p[205] = [0.0, 0.0, 110.0]            # (with leaf 1e-4 it would be outside; here it is a voxel of its own: A B A)
    out["interrupted"] = p
    return out


PATTERNS = run_patterns()
N_VOX = {"one_run_of_64": 71, "one_voxel": 1, "all_alone": 1000, "a_b_a": 2, "a_b_a_b": 2, "lane_63_64": 190, "thread_255_256": 588, "interrupted": 271}


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_runs_inside_and_across_wavefronts_combined_and_plain(name):
    pose = np.array([[0.0, 0, 0, 1.0, 0, 0, 2.0]])
    got, model = both_forms(PATTERNS[name] - [0, 0, 2.0], poses=pose, what=name, leaf=1.0, min_range=0.1)
    assert got[3] == N_VOX[name]
    if name == "a_b_a":
        assert model.wave_claims == 3 and got[0]["count"].tolist() == [9, 7]
    if name == "one_run_of_64":
        assert model.wave_claims == 64 + 1 + 6


def test_a_point_out_of_voxel_range_on_one_axis_leaves_nothing_in_the_run_before_it():
    """Such a point has offsets and view terms on its other axes and carries the number of the run before it: all thirteen of its
    values must be zeros."""
    leaf = 1e-4  # voxels reach to +-104.86 m, max_range 120 m lets a point at x = 110 m through to the voxel step
    a = np.array([[1.03005, 1.03005, 1.03005], [1.03007, 1.03006, 1.03008]])
    b = np.array([[2.00011, 2.00012, 2.00013], [2.00015, 2.00017, 2.00019], [2.00012, 2.00018, 2.00016]])
    x = np.array([[110.000037, 1.070053, 1.090071], [1.050041, -108.000029, 1.030067], [1.010013, 1.020059, 111.000083]])
    filler = _own(np.arange(40))
    cases = {
        "behind_a_run": np.concatenate([a, x[:1]]),
        "three_behind_a_run": np.concatenate([b, x]),
        "inside_a_voxels_points": np.concatenate([a[:1], a[1:], x[1:2], a[::-1]]),
        "in_front_and_behind": np.concatenate([x[2:], a, x[:2], b, x]),
        "across_lane_63_64": np.concatenate([filler, filler[:22] + [0.0, 70.0, 0.0], b[:2], x, b[2:], a, x[:1]]),
    }
    for name, pts in cases.items():
        for pose in (None, np.array([[0.0, 0, 0, 1.0, 0.00001, 0.00002, -0.00001]])):
            _, model = both_forms(pts, poses=pose, what=name, leaf=leaf, min_range=0.1, max_range=120.0)
            assert model.outside == int((np.abs(pts) > 100).any(axis=1).sum()) > 0


def test_every_kind_of_dropped_point_is_counted_in_its_own_word_and_keeps_its_index():
    lo, hi = 0.5, 40.0
    a = np.array([[0, 0, 0], [1, 1, 1], [np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [0, 0, 0],
                  [lo, 0, 0], [np.nextafter(lo, 0), 0, 0], [0, np.nextafter(lo, 1), 0],
                  [0, 0, hi], [0, 0, np.nextafter(hi, np.inf)], [np.nextafter(hi, 0), 0, 0], [1e200, 0, 0], [2, 2, 2]], dtype=np.float64)
    b = np.array([[1, 2, 3], [0, 0, 0], [3, 2, 1]], dtype=np.float64)   # at a pose that carries them out of the voxel range
    pts, offsets = np.concatenate([a, b, a]), [0, len(a), len(a) + len(b), 2 * len(a) + len(b)]
    poses = np.array([[0, 0, 0, 1.0, 0, 0, 0], [0, 0, 0, 1.0, 3e5, 0, 0], [0, 0, 0, 1.0, 0.25, 0, 0]])
    got, model = both_forms(pts, offsets, poses, what="drops", leaf=0.2, min_range=lo, max_range=hi)
    assert (model.invalid, model.range, model.outside, model.used) == (8, 9, 2, 12)
    assert got[0]["first"].tolist() == [1, 6, 8, 9, 11, 13, 18, 23, 25, 26, 28, 30]


# ---- 4. two adds, clear ------------------------------------------------------------------------------------------------------------
def test_two_adds_equal_one_add_and_a_cleared_map_is_a_fresh_one():
    rng = np.random.default_rng(46)
    first_call = rng.uniform(-5, 5, (3000, 3))
    second_call = np.concatenate([rng.uniform(-5, 5, (1500, 3)), rng.uniform(5, 9, (1500, 3))])[rng.permutation(3000)]
    poses = np.stack([small_pose(rng, angle=0.05, shift=0.5) for _ in range(2)])
    m, model = make(max_voxels=1 << 15)
    one, _ = make(max_voxels=1 << 15)
    try:
        dev_add(m, first_call, poses=poses[:1])
        model.add(first_call, poses=poses[:1])
        f1 = check(m, model, "first call")
        dev_add(m, second_call, poses=poses[1:])
        model.add(second_call, poses=poses[1:])
        e1 = check(m, model, "both calls")
        n1 = f1[3]
        assert M.same_bytes(e1[0]["first"][:n1], f1[0]["first"]) and (e1[0]["first"][n1:] >= 3000).all() and e1[3] > n1
        dev_add(one, np.concatenate([first_call, second_call]), [0, 3000, 6000], poses)
        e2 = dev_emit(one)
        M.assert_records_equal(e2[0], e1[0], "two adds and one add")
        M.assert_stats_equal(one.stats(), m.stats())
        m.clear()
        M.assert_stats_equal(m.stats(), M.SurfelMapModel().stats(), "cleared")
        assert dev_emit(m)[3] == 0 and m.claims() == 0
        dev_add(m, np.concatenate([first_call, second_call]), [0, 3000, 6000], poses)
        M.assert_records_equal(dev_emit(m)[0], e1[0], "refilled")
        M.assert_stats_equal(one.stats(), m.stats())
    finally:
        m.close(), one.close()


# ---- 5. emit -------------------------------------------------------------------------------------------------------------------------
def test_emit_by_min_points_capacity_and_optional_outputs():
    rng = np.random.default_rng(47)
    pts = rng.normal(size=(300, 3)) * [0.8, 0.8, 0.2]
    m, model = make(leaf=0.5, min_range=0.0, max_voxels=256)
    try:
        dev_add(m, pts)
        model.add(pts)
        full = model.emit()
        top = int(full[0]["count"].max())
        assert top >= 3 and (full[0]["count"] == 1).any() and 10 < full[1] <= 128
        for min_points in (0, 1, 2, top, top + 1, 0xFFFFFFFF):
            got = check(m, model, min_points, min_points=min_points)
            assert (got[3] == 0) == (min_points > top) and (min_points > 1 or got[3] == full[1])
        for min_points in (1, 2):
            n = model.emit(min_points)[1]
            for capacity in range(0, n + 2):
                check_emit(dev_emit(m, min_points, capacity), model.emit(min_points, capacity), (min_points, capacity))
        want = model.emit(2, 5)
        for rec in (False, True):
            for xyz in (False, True):
                for normal in (False, True):
                    check_emit(dev_emit(m, 2, 5, rec, xyz, normal), want, (rec, xyz, normal))
        check_emit(dev_emit(m), model.emit())  # emit does not change the map
        M.assert_stats_equal(m.stats(), model.stats())
        # the host form
        M.assert_emit_equal(m.emit(2, capacity=5), want, "host emit")
        M.assert_emit_equal(m.emit(), full, "host emit, everything")
        assert m.emit(1, capacity=0)[1] == full[1]
    finally:
        m.close()


def test_the_host_add_equals_the_device_add():
    rng = np.random.default_rng(48)
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


# ---- 6. overflow -----------------------------------------------------------------------------------------------------------------------
def test_a_map_too_small_says_so_and_works_again_after_clear():
    pts = _own(np.arange(100))
    m, _ = make(leaf=1.0, min_range=0.1, max_voxels=8)
    try:
        for plain in (0, 1):
            with option("NO_SURFEL_COMBINE", plain):
                dev_add(m, pts)
            st = m.stats()
            assert int(st["overflow"]) > 0 and int(st["voxels"]) <= 8 and int(st["points_offered"]) == 100 * (plain + 1)
            assert dev_emit(m)[3] <= 8
            dev_query(m, pts)
        m.clear()
        model = M.SurfelMapModel(1.0, 0.1, 120.0)
        dev_add(m, pts[:8])
        model.add(pts[:8])
        check(m, model, "after clear")
    finally:
        m.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
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
            c.surfel_map(capi.SurfelMapParams(leaf, lo, hi), max_voxels).close()
        return status_of(go)

    assert create() == capi.OK and create(lo=0.0, hi=0.0) == capi.OK
    for kw in (dict(leaf=0.0), dict(leaf=-1.0), dict(leaf=nan), dict(leaf=inf), dict(lo=-0.1), dict(lo=nan), dict(lo=inf), dict(hi=0.4),
               dict(hi=nan), dict(max_voxels=0)):
        assert create(**kw) == capi.ERR_BAD_PARAM, kw
    assert create(max_voxels=(1 << 30) + 1) == capi.ERR_UNSUPPORTED
    lib, szp = c.lib, C.POINTER(C.c_size_t)
    st = capi.SurfelMapParams().struct()
    h = C.c_void_p()
    assert lib.loamx_surfel_map_create(c.h, None, 64, C.byref(h)) == capi.ERR_BAD_PARAM
    assert lib.loamx_surfel_map_create(c.h, C.byref(st), 64, None) == capi.ERR_BAD_PARAM
    assert lib.loamx_surfel_map_create(None, C.byref(st), 64, C.byref(h)) == capi.ERR_BAD_PARAM

    rng = np.random.default_rng(49)
    pts = rng.uniform(-5, 5, (500, 3))
    m, model = make()
    d_pts, d_out = c.alloc(pts.nbytes).upload(pts), c.alloc(4096)
    try:
        dev_add(m, pts)
        model.add(pts)
        before = check(m, model)
        claims = m.claims()
        one = np.array([0, 500], dtype=np.uint64)
        assert status_of(m.add_clouds_dev, d_pts.ptr, 2, one) == capi.ERR_BAD_PARAM                  # point_stride < 3
        assert status_of(m.add_clouds_dev, d_pts.ptr, 1 << 32, one) == capi.ERR_UNSUPPORTED
        assert status_of(m.add_clouds_dev, d_pts.ptr, 3, [0, 300, 200, 500]) == capi.ERR_BAD_PARAM  # descending offsets
        assert status_of(m.add_clouds_dev, 0, 3, one) == capi.ERR_BAD_PARAM                           # null points
        assert lib.loamx_surfel_map_add_clouds(c.h, m.h, d_pts.ptr, 3, None, 1, None) == capi.ERR_BAD_PARAM  # null offsets
        assert lib.loamx_surfel_map_add_clouds(c.h, None, d_pts.ptr, 3, one.ctypes.data_as(szp), 1, None) == capi.ERR_BAD_PARAM
        assert lib.loamx_surfel_map_add_clouds_f32(c.h, None, d_pts.ptr, 3, one.ctypes.data_as(szp), 1, None) == capi.ERR_BAD_PARAM
        assert lib.loamx_surfel_map_add_cloud_host(c.h, m.h, None, 3, 5, None) == capi.ERR_BAD_PARAM
        assert lib.loamx_surfel_map_add_cloud_host_f32(c.h, m.h, None, 3, 5, None) == capi.ERR_BAD_PARAM
        # the 2^32 - 2 total: in one call, and together with what the map already took (the call is refused before anything is read)
        assert status_of(m.add_clouds_dev, d_pts.ptr, 3, [0, (1 << 32) - 1]) == capi.ERR_UNSUPPORTED
        assert status_of(m.add_clouds_dev, d_pts.ptr, 3, [0, (1 << 32) - 2 - 499]) == capi.ERR_UNSUPPORTED
        with pytest.raises(ValueError):
            m.add_clouds_dev(d_pts.ptr, 3, [0, -5])
        assert status_of(m.emit_dev, 10, 0, 1, d_out.ptr) == capi.ERR_BAD_PARAM    # null d_n_out
        assert lib.loamx_surfel_map_emit(c.h, None, 1, None, None, None, 0, d_out.ptr) == capi.ERR_BAD_PARAM
        n_host = C.c_size_t(0)
        assert lib.loamx_surfel_map_emit_host(c.h, m.h, 1, None, 10, C.byref(n_host)) == capi.ERR_BAD_PARAM
        assert lib.loamx_surfel_map_emit_host(c.h, m.h, 1, None, 0, None) == capi.ERR_BAD_PARAM
        assert status_of(m.query_dev, 0, 3, 5, 1, d_out.ptr) == capi.ERR_BAD_PARAM            # null points
        assert status_of(m.query_dev, d_pts.ptr, 2, 5, 1, d_out.ptr) == capi.ERR_BAD_PARAM    # point_stride < 3
        assert status_of(m.query_dev, d_pts.ptr, 1 << 32, 5, 1, d_out.ptr) == capi.ERR_UNSUPPORTED
        assert status_of(m.query_dev, d_pts.ptr, 3, (1 << 31) + 1, 1, d_out.ptr) == capi.ERR_UNSUPPORTED
        assert lib.loamx_surfel_map_query(c.h, None, d_pts.ptr, 3, 5, 1, None, None, None) == capi.ERR_BAD_PARAM
        assert lib.loamx_surfel_map_stats_read(c.h, m.h, None) == capi.ERR_BAD_PARAM
        assert lib.loamx_surfel_map_claims_read(c.h, m.h, None) == capi.ERR_BAD_PARAM
        assert lib.loamx_surfel_map_clear(c.h, None) == capi.ERR_BAD_PARAM
        with pytest.raises(ValueError):
            m.emit_dev(-1, d_out.ptr)
        with pytest.raises(ValueError):
            m.query(np.zeros((4, 2)))
        M.assert_records_equal(dev_emit(m)[0], before[0], "after the refusals")
        M.assert_stats_equal(m.stats(), model.stats(), "after the refusals")
        assert m.claims() == claims
        assert status_of(m.add_clouds_dev, d_pts.ptr, 3, [0, 0]) == capi.OK and status_of(m.add_clouds_dev, 0, 3, [7]) == capi.OK  # nothing to add
        assert status_of(m.query_dev, 0, 3, 0, 1, d_out.ptr) == capi.OK
        M.assert_stats_equal(m.stats(), model.stats(), "after the empty calls")
    finally:
        d_pts.free(), d_out.free(), m.close()
    with pytest.raises(ValueError):
        m.clear()  # closed


def test_a_map_belongs_to_the_context_that_created_it():
    m, model = make()
    other = capi.Context(0)
    d_out = other.alloc(1024)
    try:
        pts = np.random.default_rng(50).uniform(-3, 3, (200, 3))
        dev_add(m, pts)
        model.add(pts)
        lib = other.lib
        off = np.array([0, 1], dtype=np.uint64)
        szp = off.ctypes.data_as(C.POINTER(C.c_size_t))
        assert lib.loamx_surfel_map_clear(other.h, m.h) == capi.ERR_BAD_PARAM
        assert lib.loamx_surfel_map_add_clouds(other.h, m.h, d_out.ptr, 3, szp, 1, None) == capi.ERR_BAD_PARAM
        assert lib.loamx_surfel_map_add_clouds_f32(other.h, m.h, d_out.ptr, 3, szp, 1, None) == capi.ERR_BAD_PARAM
        assert lib.loamx_surfel_map_emit(other.h, m.h, 1, d_out.ptr, None, None, 1, d_out.ptr) == capi.ERR_BAD_PARAM
        assert lib.loamx_surfel_map_query(other.h, m.h, d_out.ptr, 3, 1, 1, d_out.ptr, None, None) == capi.ERR_BAD_PARAM
        st = np.zeros(1, dtype=capi.SURFEL_MAP_STATS_DTYPE)
        assert lib.loamx_surfel_map_stats_read(other.h, m.h, st.ctypes.data) == capi.ERR_BAD_PARAM
        n = C.c_uint64(0)
        assert lib.loamx_surfel_map_claims_read(other.h, m.h, C.byref(n)) == capi.ERR_BAD_PARAM
        check(m, model, "after the other context's calls")
    finally:
        d_out.free(), other.close(), m.close()


# ---- 8. query ------------------------------------------------------------------------------------------------------------------------
def test_query_finds_the_records_of_the_maps_own_means_and_nothing_elsewhere():
    rng = np.random.default_rng(51)
    pts = rng.normal(size=(3000, 3)) * [3.0, 3.0, 0.4]
    pose = small_pose(rng, angle=0.3, shift=1.0)
    m, model = make(leaf=0.5)
    try:
        dev_add(m, pts, poses=pose[None])
        model.add(pts, poses=pose[None])
        rec, n = model.emit()
        means = np.ascontiguousarray(rec["mean"])
        got = dev_query(m, means)
        M.assert_records_equal(got[0], rec, "own means")  # (a mean lies in its own voxel)
        check_query(got, model.query(means), "own means")
        assert np.abs(got[1]).max() < 1e-12 and M.same_bytes(got[2], rec["count"])
        # the cloud's own points at their poses, points without a voxel, out of range and not finite; stride 5
        world = CM.pose_act(pose, pts[:500])
        far = np.array([[50.0, 50.0, 50.0], [-0.25, 77.0, 0.1], [0.5 * (1 << 20), 0, 0], [0, -0.5 * (1 << 20) - 1, 0], [np.nan, 0, 0], [0, np.inf, 0]])
        q = np.full((506, 5), np.nan)
        q[:, :3] = np.concatenate([world, far])
        for min_points in (0, 1, 2, 3, 1000):
            got = dev_query(m, q, min_points)
            want = model.query(q, min_points)
            check_query(got, want, min_points)
            assert not got[2][500:].any() and not got[1][500:].any() and not got[0][500:].tobytes().strip(b"\0")
        below = model.query(q, 3)[2][:500] == 0
        assert below.any() and not below.all() and (model.query(q, 1)[2][:500] > 0).all()  # voxels below min_points read as nothing
        assert np.abs(model.query(q, 1)[1][:500]).max() > 1e-3
        want = model.query(q, 2)
        for rec_on in (False, True):
            for dist_on in (False, True):
                for cnt_on in (False, True):
                    check_query(dev_query(m, q, 2, rec_on, dist_on, cnt_on), want, (rec_on, dist_on, cnt_on))
        host = m.query(q, 2)
        check_query(host, want, "host query")
        M.assert_stats_equal(m.stats(), model.stats(), "a query changes nothing")
    finally:
        m.close()


def test_at_equal_leaf_the_voxels_are_the_cloud_maps_in_the_same_order():
    rng = np.random.default_rng(52)
    calls = [(rng.uniform(-6, 6, (2500, 3)), [0, 1000, 1000, 2500], np.stack([small_pose(rng, 0.2, 1.0) for _ in range(3)])),
             (rng.uniform(-9, 9, (1500, 3)).astype(np.float32), [0, 1500], None)]
    c = ctx()
    sm = c.surfel_map(capi.SurfelMapParams(0.4, 0.5, 120.0), 1 << 14)
    cm = c.cloud_map(capi.CloudMapParams(0.4, 0.5, 120.0), 1 << 14)
    try:
        for pts, off, poses in calls:
            for m in (sm, cm):
                dev_add(m, pts, off, poses)
        for min_points in (1, 3):
            rec, n = sm.emit(min_points)
            xyz, count, first, n_cloud = cm.emit(min_points)
            assert n == n_cloud > (1000 if min_points == 1 else 0) and M.same_bytes(rec["count"], count) and M.same_bytes(rec["first"], first)
            # the same voxels: the surfel mean is the centroid quantised to leaf / 65536
            assert np.array_equal(np.floor(rec["mean"] / 0.4), np.floor(xyz / 0.4)) and np.abs(rec["mean"] - xyz).max() <= 0.4 / 65536
        assert {k: int(sm.stats()[k]) for k in M.STAT_NAMES} == {k: int(cm.stats()[k]) for k in M.STAT_NAMES}
        assert sm.claims() == cm.claims()
    finally:
        sm.close(), cm.close()


# ---- 9. an organised scan through the chain ------------------------------------------------------------------------------------------
def test_a_lot_scan_from_organize_to_query_without_a_synchronise():
    import organize_common as OC
    c = ctx()
    H, W, leaf = 16, 256, 4.0  # (sixteen beams 1.8 degrees apart: a box face at 20 m is hit every 0.6 m upwards)
    origin, yaw = S.sensor_origin("lot", 0)
    scan = S.scan_at("lot", 0, origin, yaw, H=H, W=W)
    cloud = scan[np.random.default_rng(53).permutation(H * W)]
    lidar = capi.LidarParams(H, W, 1.0, 120.0)
    lay = c.scan_layout(lidar, capi.OrganizeParams(elevations=OC.fan_elevations(H, S.FANS["lot"])))
    results = np.zeros(1, dtype=capi.RESULT_DTYPE)
    results["pose"] = [S.yaw_pose(0.0, [0.0, 0.0, 0.0])]
    n = H * W
    bufs = [c.alloc(cloud.nbytes).upload(cloud), c.alloc(n * 24), c.alloc(results.nbytes).upload(results), c.alloc(2 * 56),
            poisoned(c, n * REC), poisoned(c, 16), c.alloc(n * 24), poisoned(c, n * REC), poisoned(c, n * 8), poisoned(c, n * 4)]
    d_cloud, d_scan, d_results, d_traj, d_rec, d_n, d_world, d_qrec, d_qdist, d_qcnt = bufs
    m, model = make(leaf=leaf, max_voxels=1 << 13)
    try:
        # the scan's own points in the world frame, the positions of the query, are uploaded before the chain starts
        organised_world = S.to_world(scan, origin, yaw)
        d_world.upload(organised_world)
        c.organize_clouds_dev(lay, d_cloud.ptr, 3, [0, n], d_scan.ptr)
        c.compose_trajectory_dev(d_results.ptr, 1, d_traj.ptr, origin=S.yaw_pose(yaw, origin))
        m.add_clouds_dev(d_scan.ptr, 3, [0, n], d_traj.ptr + 56)
        m.emit_dev(n, d_n.ptr, 3, d_rec.ptr)
        m.query_dev(d_world.ptr, 3, n, 3, d_qrec.ptr, d_qdist.ptr, d_qcnt.ptr)
        c.synchronize()
        organised = d_scan.download(np.float64, n * 3).reshape(-1, 3)
        traj = d_traj.download(np.float64, 14).reshape(2, 7)
        model.add(organised, poses=traj[1:2])
        # asserted on the model first: wall voxels (no ground in them, hits of more than one scan line, six points or more) face the
        # sensor, and those among them that hold one face of a box are flat with a horizontal normal; ground voxels look up
        every, _ = model.emit(1)
        world = CM.pose_act(traj[1], organised)
        what, _, key, _, _ = M.point_terms(organised, traj[1], leaf, model.min_range, model.max_range)
        zs = {}
        for k, z in zip(key[what == CM.USED].tolist(), world[what == CM.USED, 2].tolist()):
            zs.setdefault(k, []).append(z)
        z_lo, z_hi = (np.array([f(zs[k]) for k in model.vox]) for f in (min, max))
        wall = (z_lo > 0.3) & (z_hi - z_lo > 0.5) & (every["count"] >= 6)
        ground = (z_hi < 0.1) & (every["count"] >= 6)
        flat = every["eval"][:, 0] <= 0.02 * every["eval"][:, 2]
        facing = (every["normal"] * (origin[None, :] - every["mean"])).sum(axis=1) > 0.0
        assert wall.sum() >= 8 and (wall & flat).sum() >= 6 and facing[wall].all(), (int(wall.sum()), int((wall & flat).sum()))
        assert (np.abs(every["normal"][wall & flat, 2]) < 0.1).all()
        assert ground.sum() >= 20 and (every["normal"][ground, 2] > 0.99).all() and flat[ground].all(), int(ground.sum())
        want, n_want = model.emit(3)
        got_n = int(d_n.download(np.uint32, 1)[0])
        assert got_n == n_want > 200
        M.assert_records_equal(d_rec.download(M.SURFEL_DTYPE, n)[:got_n], want, "chain emit")
        assert is_poison(d_rec.download(M.SURFEL_DTYPE, n)[got_n:])
        check_query((d_qrec.download(M.SURFEL_DTYPE, n), d_qdist.download(np.float64, n), d_qcnt.download(np.uint32, n)),
                    model.query(organised_world, 3), "chain query")
        M.assert_stats_equal(m.stats(), model.stats())
    finally:
        for b in bufs:
            b.free()
        m.close(), lay.close()
