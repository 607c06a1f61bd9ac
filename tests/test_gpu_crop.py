"""GPU: the map window (include/loamx.h, "map window"; loam_amd/csrc/crop_kernels.hip) of the cloud map, the surfel map and the
occupancy map against the models of tests/cloudmap_common.py, tests/surfel_common.py and tests/occupancy_common.py with the removed
entries deleted (tests/crop_common.py), by equality of bytes: emit, query, box, slice and the stats. The counts word goes into a
poisoned buffer. Every case runs for the three maps unless its name says otherwise."""
import copy
import ctypes as C

import numpy as np
import pytest

import cloudmap_common as CM
import crop_common as X
import localize_common as L
import occupancy_common as OM
import surfel_common as SM
from gpu_common import ctx, option
from loam_amd import capi

pytestmark = pytest.mark.gpu

KINDS = ("cloud", "surfel", "occupancy")
NO_COMBINE = {"cloud": "NO_CLOUDMAP_COMBINE", "surfel": "NO_SURFEL_COMBINE", "occupancy": "NO_OCCUPANCY_COMBINE"}
POISON = 0xA5
POISON_U32 = np.uint32(0xA5A5A5A5)
INF = np.inf
WIDE = 1.0e6
UNIT_Q = [0.0, 0.0, 0.0, 1.0]


# ---- the three maps behind one face ------------------------------------------------------------------------------------------------
def make(kind, max_voxels, leaf=0.5, min_range=0.01, max_range=80.0, c=None):
    """(device map, model)"""
    c = c or ctx()
    if kind == "cloud":
        return c.cloud_map(capi.CloudMapParams(leaf, min_range, max_range), max_voxels), CM.CloudMapModel(leaf, min_range, max_range)
    if kind == "surfel":
        return c.surfel_map(capi.SurfelMapParams(leaf, min_range, max_range), max_voxels), SM.SurfelMapModel(leaf, min_range, max_range)
    return (c.occupancy_map(capi.OccupancyParams(leaf=leaf, min_range=min_range, max_range=max_range), max_voxels),
            OM.OccupancyModel(leaf=leaf, min_range=min_range, max_range=max_range))


def dev_add(m, pts, offsets=None, poses=None):
    """uploads the clouds and their poses and adds them through the device entry point (one call)"""
    c = m.ctx
    pts = np.ascontiguousarray(pts)
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


def add(m, model, pts, offsets=None, poses=None):
    dev_add(m, pts, offsets, poses)
    model.add(pts, offsets, poses)


def stats_of(kind, st):
    names = OM.STAT_NAMES if kind == "occupancy" else CM.STAT_NAMES
    return {n: int(st[n]) for n in names}


def readout(kind, m, probe):
    """every read-out of the map as a list of (name, value): probe = dict(points (n, 3), vmin, dims)"""
    if kind == "cloud":
        xyz, cnt, first, n = m.emit()
        out = [("n", n), ("xyz", xyz), ("count", cnt), ("first", first)]
    elif kind == "surfel":
        rec, n = m.emit()
        q = m.query(probe["points"])
        out = [("n", n), ("records", rec), ("query records", q[0]), ("query distance", q[1]), ("query count", q[2])]
    else:
        counts, state = m.box(probe["vmin"], probe["dims"])
        qc, qs = m.query(probe["points"])
        out = [("box counts", counts), ("box state", state), ("slice", m.slice(probe["vmin"], probe["dims"])), ("query counts", qc),
               ("query state", qs)]
    return out + [("stats", stats_of(kind, m.stats()))]


def expected(kind, model, probe):
    if kind == "cloud":
        xyz, cnt, first, n = model.emit()
        out = [("n", n), ("xyz", xyz), ("count", cnt), ("first", first)]
    elif kind == "surfel":
        rec, n = model.emit()
        q = model.query(probe["points"])
        out = [("n", n), ("records", rec), ("query records", q[0]), ("query distance", q[1]), ("query count", q[2])]
    else:
        counts, state = model.box(probe["vmin"], probe["dims"])
        qc, qs = model.query(probe["points"])
        out = [("box counts", counts), ("box state", state), ("slice", model.slice(probe["vmin"], probe["dims"])), ("query counts", qc),
               ("query state", qs)]
    return out + [("stats", stats_of(kind, model.stats()))]


def assert_same(got, want, what=""):
    assert [g[0] for g in got] == [w[0] for w in want]
    for (name, g), (_, w) in zip(got, want):
        if isinstance(w, np.ndarray):
            assert CM.same_bytes(g, w), (what, name, getattr(g, "shape", None), w.shape)
        else:
            assert g == w, (what, name, g, w)


def check(kind, m, model, probe, what=""):
    got = readout(kind, m, probe)
    assert_same(got, expected(kind, model, probe), what)
    return got


def device_pose(c, pose):
    return c.alloc(56).upload(np.ascontiguousarray(pose, dtype=np.float64))


def dev_crop(m, lo, hi, pose=None, with_counts=True):
    """crop_dev with the pose in device memory (None: no pose) and a poisoned counts buffer of eight words -> the four counts,
    after checking that the four words behind them are still poison; with_counts False: no counts asked for, None"""
    c = m.ctx
    d_pose = device_pose(c, pose) if pose is not None else None
    d_counts = c.alloc(32).upload(np.full(32, POISON, dtype=np.uint8))
    try:
        m.crop_dev(lo, hi, d_pose.ptr if d_pose else 0, d_counts.ptr if with_counts else 0)
        c.synchronize()
        words = d_counts.download(np.uint32, 8)
    finally:
        d_counts.free()
        if d_pose:
            d_pose.free()
    assert (words[4 if with_counts else 0:] == POISON_U32).all(), words
    return [int(w) for w in words[:4]] if with_counts else None


def crop(kind, m, model, lo, hi, pose=None, what=""):
    """the device crop and the model's; their counts agree"""
    counts = dev_crop(m, lo, hi, pose)
    kept, removed, skipped = X.crop_model(model, pose, lo, hi)
    assert counts == [kept, removed, skipped, 0], (what, counts, kept, removed, skipped)
    return counts


# ---- one voxel per cloud: a point 0.1 in front of a sensor that the pose places inside the voxel. The occupancy map's ray then visits
# no other voxel (its walk would end 0.2 in front of the return, that is, behind the sensor: there is no walk). --------------------------
def cell_cloud(cells, leaf):
    """(points (n, 3), offsets, poses (n, 7)): one cloud of one point per cell, the point at the cell's centre"""
    cells = np.asarray(cells, dtype=np.float64).reshape(-1, 3)
    poses = np.zeros((len(cells), 7))
    poses[:, 3] = 1.0
    poses[:, 4:] = (cells + 0.5) * leaf - [0.1, 0.0, 0.0]
    return np.tile([0.1, 0.0, 0.0], (len(cells), 1)), np.arange(len(cells) + 1), poses


def add_cells(m, model, cells, leaf):
    pts, off, poses = cell_cloud(cells, leaf)
    add(m, model, pts, off, poses)


def centres(cells, leaf):
    return (np.asarray(cells, dtype=np.float64).reshape(-1, 3) + 0.5) * leaf


# ---- 1. probe chains -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_voxels_behind_a_removed_one_in_a_probe_chain_are_still_found(kind):
    """what a delete that empties a slot gets wrong: A, B, C, D share a home slot and entered in that order, A and B leave"""
    log2_cap = X.table_log2(2 * 8)
    assert log2_cap == 4
    cells = X.colliding_cells(4, log2_cap)
    keys = [X.cell_key(c) for c in cells]
    assert len(set(keys)) == 4 and len({X.home_slot(k, log2_cap) for k in keys}) == 1
    assert all(c[1] == 0 and c[2] == 0 for c in cells) and cells[0][0] < cells[1][0] < cells[2][0] < cells[3][0]
    a, b, c_, d = cells
    leaf = 1.0
    m, model = make(kind, 8, leaf=leaf)
    probe = dict(points=centres(cells + [(0, 0, 0)], leaf), vmin=np.array([-1, -1, -1], dtype=np.int32),
                 dims=np.array([cells[3][0] + 3, 3, 3], dtype=np.uint32))
    try:
        for cell in cells:  # a call each: the insertion order, and with it the chain, is certain
            add_cells(m, model, [cell], leaf)
        check(kind, m, model, probe, "before")
        lo, hi = [b[0] * leaf + 1.0, -WIDE, -WIDE], [WIDE, WIDE, WIDE]  # from the cell behind B onwards
        assert crop(kind, m, model, lo, hi) == [2, 2, 0, 0]
        assert list(model.vox) == keys[2:]
        got = dict(check(kind, m, model, probe, "A and B removed"))
        if kind == "cloud":
            assert got["first"].tolist() == [2, 3] and got["n"] == 2
        elif kind == "surfel":
            assert got["records"]["first"].tolist() == [2, 3] and got["query count"].tolist() == [0, 0, 1, 1, 0]
        else:
            assert got["query counts"].tolist() == [[0, 0], [0, 0], [1, 0], [1, 0], [0, 0]] and (got["query state"][:2] == OM.UNKNOWN).all()
        add_cells(m, model, [a], leaf)  # A again: a new voxel, listed last, first = the running index
        got = dict(check(kind, m, model, probe, "A again"))
        assert list(model.vox) == keys[2:] + keys[:1]
        if kind == "cloud":
            assert got["first"].tolist() == [2, 3, 4]
        elif kind == "surfel":
            assert got["records"]["first"].tolist() == [2, 3, 4] and got["query count"].tolist() == [1, 0, 1, 1, 0]
        else:
            assert got["query counts"][:, 0].tolist() == [1, 0, 1, 1, 0]
    finally:
        m.close()


# ---- 2. tile boundaries ----------------------------------------------------------------------------------------------------------------
LINE = 600
_line_models = {}


def line_model(kind):
    """the model of LINE single-point voxels along x at leaf 1 (built once per kind; callers take a copy)"""
    if kind not in _line_models:
        model = make_model(kind, 1.0)
        model.add(*cell_cloud([(x, 0, 0) for x in range(LINE)], 1.0))
        _line_models[kind] = model
    return copy.deepcopy(_line_models[kind])


def make_model(kind, leaf, min_range=0.01, max_range=80.0):
    if kind == "cloud":
        return CM.CloudMapModel(leaf, min_range, max_range)
    if kind == "surfel":
        return SM.SurfelMapModel(leaf, min_range, max_range)
    return OM.OccupancyModel(leaf=leaf, min_range=min_range, max_range=max_range)


@pytest.mark.parametrize("kind", KINDS)
def test_boxes_that_keep_counts_around_the_tiles_of_the_compaction(kind):
    m, _ = make(kind, 1024, leaf=1.0)
    marks = sorted({0, 1, 254, 255, 256, 257, 511, 512, 513, 598, 599} | set(range(3, LINE, 37)))
    probe = dict(points=centres([(x, 0, 0) for x in marks], 1.0), vmin=np.array([-2, -1, -1], dtype=np.int32),
                 dims=np.array([LINE + 4, 3, 3], dtype=np.uint32))
    pts, off, poses = cell_cloud([(x, 0, 0) for x in range(LINE)], 1.0)
    try:
        for keep in (0, 1, 255, 256, 257, 513, LINE):
            m.clear()
            dev_add(m, pts, off, poses)
            model = line_model(kind)
            lo, hi = ([-5.0, -WIDE, -WIDE], [-1.5, WIDE, WIDE]) if keep == 0 else ([0.0, -INF, -INF], [keep - 0.5, INF, INF])
            assert crop(kind, m, model, lo, hi, what=keep) == [keep, LINE - keep, 0, 0]
            check(kind, m, model, probe, f"keeps {keep}")
        # the voxels from the middle of the list, kept by a window around a device pose
        m.clear()
        dev_add(m, pts, off, poses)
        model = line_model(kind)
        pose = np.array([0.3, 0.1, -0.2, 0.9, 300.5, 0.5, 0.5])
        assert crop(kind, m, model, [-44.0, -1.0, -1.0], [212.25, 1.0, 1.0], pose) == [257, LINE - 257, 0, 0]
        check(kind, m, model, probe, "the middle")
    finally:
        m.close()


@pytest.mark.parametrize("kind", KINDS)
def test_an_empty_map_and_a_crop_that_removes_nothing(kind):
    m, model = make(kind, 1024, leaf=1.0)
    probe = dict(points=centres([(x, 0, 0) for x in (0, 5, 299)], 1.0), vmin=np.array([-2, -1, -1], dtype=np.int32),
                 dims=np.array([304, 3, 3], dtype=np.uint32))
    try:
        assert crop(kind, m, model, [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]) == [0, 0, 0, 0]
        check(kind, m, model, probe, "empty")
        add_cells(m, model, [(x, 0, 0) for x in range(300)], 1.0)
        before = readout(kind, m, probe)
        assert crop(kind, m, model, [-INF] * 3, [INF] * 3) == [300, 0, 0, 0]
        assert_same(readout(kind, m, probe), before, "all six bounds infinite")
        assert crop(kind, m, model, [0.0, 0.0, 0.0], [299.5, 0.5, 0.5]) == [300, 0, 0, 0]
        assert_same(readout(kind, m, probe), before, "a box that holds every voxel")
        check(kind, m, model, probe, "nothing removed")
    finally:
        m.close()


# ---- 3. against the model --------------------------------------------------------------------------------------------------------------
posed_clouds = X.posed_clouds


def probe_of(model, pts, offsets, poses, every=23, pad=2):
    """query points (the clouds' points in the map frame, every `every`-th) and a box around all of them"""
    moved = np.concatenate([CM.pose_act(poses[c], pts[offsets[c]:offsets[c + 1], :3].astype(np.float64)) for c in range(len(poses))])
    leaf = X.model_leaf(model)
    lo, hi = np.floor(moved.min(axis=0) / leaf) - pad, np.floor(moved.max(axis=0) / leaf) + pad
    return dict(points=np.ascontiguousarray(moved[::every]), vmin=lo.astype(np.int32), dims=(hi - lo + 1).astype(np.uint32))


@pytest.mark.parametrize("form", ["f64", "f32", "plain"])
@pytest.mark.parametrize("kind", KINDS)
def test_crops_between_adds_equal_the_model(kind, form):
    """three posed clouds, a crop through the middle around a device pose, a fourth cloud over the removed region, a second crop;
    the adds in float64, in float32 and in the one-claim-per-item form"""
    dtype = np.float32 if form == "f32" else np.float64
    (pts, off, poses), (pts4, off4, poses4) = X.case3_clouds()
    pts, pts4 = pts.astype(dtype), pts4.astype(dtype)
    m, model = make(kind, 4096)
    everything = (np.concatenate([pts, pts4]), np.concatenate([off, off4[1:] + off[-1]]), np.concatenate([poses, poses4]))
    probe = probe_of(model, *everything)
    centre = np.array([0.7, -0.1, 0.6, 0.4, *X.CASE3_CENTRE])  # (no unit quaternion: it is not looked at)
    try:
        with option(NO_COMBINE[kind], 1 if form == "plain" else 0):
            add(m, model, pts, off, poses)
            n0 = len(model.vox)
            check(kind, m, model, probe, "three clouds")
            kept, removed, _, _ = crop(kind, m, model, *X.CASE3_BOXES[0], centre)
            assert kept > n0 // 4 and removed > n0 // 4
            check(kind, m, model, probe, "first crop")
            add(m, model, pts4, off4, poses4)  # over the removed region: voxels come back as new voxels, kept ones grow
            assert len(model.vox) > kept + 50
            check(kind, m, model, probe, "fourth cloud")
            kept2, removed2, _, _ = crop(kind, m, model, *X.CASE3_BOXES[1], centre)
            assert kept2 > 50 and removed2 > 50
            check(kind, m, model, probe, "second crop")
            assert stats_of(kind, m.stats())["overflow"] == 0
    finally:
        m.close()


# ---- 4. room regained ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_a_crop_regains_the_room_of_the_removed_voxels(kind):
    """max_voxels = 64 filled exactly, cropped to 20, then 44 new voxels: no overflow, all 64 listed in the model's order. The same
    adds without the crop overflow. The occupancy map has no list and gives up only when its table is full: its numbers are the
    table's 128 slots filled exactly, cropped to 20, then 108 new voxels."""
    full = 128 if kind == "occupancy" else 64
    assert 1 << X.table_log2(2 * 64) == 128
    m, model = make(kind, 64, leaf=1.0)
    m2, _ = make(kind, 64, leaf=1.0)
    first, second = [(x, 0, 0) for x in range(full)], [(x, 2, 0) for x in range(100, 100 + full - 20)]
    probe = dict(points=centres(first[::5] + second[::5], 1.0), vmin=np.array([-1, -1, -1], dtype=np.int32),
                 dims=np.array([100 + full, 5, 3], dtype=np.uint32))
    try:
        add_cells(m, model, first, 1.0)
        dev_add(m2, *cell_cloud(first, 1.0))
        check(kind, m, model, probe, "filled exactly")
        assert stats_of(kind, m.stats())["voxels"] == full and stats_of(kind, m.stats())["overflow"] == 0
        assert crop(kind, m, model, [0.0, 0.0, 0.0], [19.5, 0.5, 0.5]) == [20, full - 20, 0, 0]
        add_cells(m, model, second, 1.0)
        got = dict(check(kind, m, model, probe, "filled again"))
        assert got["stats"]["voxels"] == full and got["stats"]["overflow"] == 0
        if kind != "occupancy":
            assert got["n"] == 64
            want_first = list(range(20)) + list(range(64, 108))
            assert (got["first"] if kind == "cloud" else got["records"]["first"]).tolist() == want_first
        dev_add(m2, *cell_cloud(second, 1.0))  # the inputs bite: without the crop they overflow
        assert stats_of(kind, m2.stats())["overflow"] > 0
    finally:
        m.close(), m2.close()


# ---- 5. skip ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_a_pose_that_is_not_finite_skips_the_crop_and_the_quaternion_is_not_looked_at(kind):
    pts, off, poses = posed_clouds(63, (400, 300))
    m, model = make(kind, 2048)
    probe = probe_of(model, pts, off, poses, every=9)
    try:
        add(m, model, pts, off, poses)
        before = readout(kind, m, probe)
        n = len(model.vox)
        assert n > 100
        lo, hi = [-0.25, -0.25, -0.25], [0.25, 0.25, 0.25]  # (a crop that is not skipped would remove nearly everything)
        for a in range(3):
            for bad in (np.nan, INF, -INF):
                pose = np.array(UNIT_Q + [0.1, 0.2, 0.05])
                pose[4 + a] = bad
                assert dev_crop(m, lo, hi, pose) == [n, 0, 1, 0], (a, bad)
                assert X.crop_model(model, pose, lo, hi) == (n, 0, 1)
                assert_same(readout(kind, m, probe), before, f"skipped: component {a} is {bad}")
        pose = np.array([np.nan, INF, -3.0, 0.0, 0.1, 0.2, 0.05])  # a quaternion of NaN, inf and no unit length, a finite translation
        kept, removed, skipped, _ = crop(kind, m, model, lo, hi, pose)
        assert skipped == 0 and removed > n // 2 and kept >= 1
        check(kind, m, model, probe, "a NaN quaternion")
    finally:
        m.close()


# ---- 6. host folding -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_a_centre_folded_in_on_the_host_gives_the_bytes_of_a_device_pose(kind):
    pts, off, poses = posed_clouds(64, (300, 200))
    m1, model = make(kind, 1 << 15, leaf=0.2)  # (0.2 is not representable: the bounds land where the division puts them)
    m2, _ = make(kind, 1 << 15, leaf=0.2)
    probe = probe_of(model, pts, off, poses, every=11)
    centre = [0.123456789, -0.3, 0.0499999]
    lo, hi = [-3.7, -2.9, -1.35], [0.7, 3.1, 1.15]
    try:
        add(m1, model, pts, off, poses)
        dev_add(m2, pts, off, poses)
        kept, removed = m1.crop(lo, hi, centre)
        counts = dev_crop(m2, lo, hi, np.array(UNIT_Q + centre))
        assert counts == [kept, removed, 0, 0] and X.crop_model(model, np.array(UNIT_Q + centre), lo, hi) == (kept, removed, 0)
        assert kept > 50 and removed > 50
        a, b = readout(kind, m1, probe), readout(kind, m2, probe)
        assert_same(a, b, "host folding against a device pose")
        assert_same(a, expected(kind, model, probe), "against the model")
        with pytest.raises(ValueError):
            m1.crop(lo, hi, [0.0, np.nan, 0.0])
        with pytest.raises(ValueError):
            m1.crop(lo, hi, [0.0, 0.0])
        with pytest.raises(ValueError):
            m1.crop_dev([0.0, 0.0], hi)
        with pytest.raises(ValueError):
            m1.crop_dev(lo, np.array(["a", "b", "c"]))
        assert_same(readout(kind, m1, probe), a, "after the ValueErrors")
    finally:
        m1.close(), m2.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_refusals_change_nothing_and_the_counts_are_optional(kind):
    pts, off, poses = posed_clouds(65, (500,))
    m, model = make(kind, 2048)
    probe = probe_of(model, pts, off, poses, every=7)
    c = m.ctx
    other = capi.Context(0)
    fn = getattr(c.lib, {"cloud": "loamx_cloud_map_crop", "surfel": "loamx_surfel_map_crop", "occupancy": "loamx_occupancy_crop"}[kind])
    d_counts = c.alloc(32).upload(np.full(32, POISON, dtype=np.uint8))
    d_other = other.alloc(32).upload(np.full(32, POISON, dtype=np.uint8))
    d_pose = device_pose(c, UNIT_Q + [0.0, 0.0, 0.0])
    vec = lambda *v: np.array(v, dtype=np.float64)
    try:
        add(m, model, pts, off, poses)
        before = readout(kind, m, probe)
        lo, hi = vec(-1.0, -1.0, -1.0), vec(1.0, 1.0, 1.0)
        call = lambda h_ctx, h_map, l, h, counts: fn(h_ctx, h_map, d_pose.ptr, None if l is None else l.ctypes.data,
                                                     None if h is None else h.ctypes.data, counts)
        assert call(c.h, None, lo, hi, d_counts.ptr) == capi.ERR_BAD_PARAM            # a null map
        assert call(c.h, m.h, None, hi, d_counts.ptr) == capi.ERR_BAD_PARAM           # null lo
        assert call(c.h, m.h, lo, None, d_counts.ptr) == capi.ERR_BAD_PARAM           # null hi
        assert fn(other.h, m.h, None, lo.ctypes.data, hi.ctypes.data, d_other.ptr) == capi.ERR_BAD_PARAM  # a map of another context
        assert b"another context" in other.lib.loamx_last_error(other.h)
        for a in range(3):
            bad_lo, bad_hi = lo.copy(), hi.copy()
            bad_lo[a] = 1.5                                                          # lo > hi
            assert call(c.h, m.h, bad_lo, hi, d_counts.ptr) == capi.ERR_BAD_PARAM
            assert b"lo <= hi" in c.lib.loamx_last_error(c.h)
            bad_lo[a] = np.nan                                                       # a NaN bound
            assert call(c.h, m.h, bad_lo, hi, d_counts.ptr) == capi.ERR_BAD_PARAM
            bad_hi[a] = np.nan
            assert call(c.h, m.h, lo, bad_hi, d_counts.ptr) == capi.ERR_BAD_PARAM
        assert fn(None, m.h, None, lo.ctypes.data, hi.ctypes.data, None) == capi.ERR_BAD_PARAM  # a null context
        c.synchronize(), other.synchronize()
        assert (d_counts.download(np.uint8, 32) == POISON).all() and (d_other.download(np.uint8, 32) == POISON).all()
        assert_same(readout(kind, m, probe), before, "after the refusals")
        # no counts asked for: the crop happens all the same
        assert dev_crop(m, lo, hi, None, with_counts=False) is None
        kept, removed, _ = X.crop_model(model, None, lo, hi)
        assert kept > 10 and removed > 10
        check(kind, m, model, probe, "without counts")
    finally:
        d_counts.free(), d_pose.free(), d_other.free(), other.close(), m.close()
    with pytest.raises(ValueError):
        m.crop_dev([0, 0, 0], [1, 1, 1])  # closed


# ---- 8. the localiser on a cropped map (surfel) -------------------------------------------------------------------------------------------
def _run(loc, scan, start):
    c = loc.ctx
    bufs = [c.alloc(scan.nbytes).upload(scan), c.alloc(56).upload(start)]
    bufs += [c.alloc(n).upload(np.full(n, POISON, dtype=np.uint8)) for n in (56, 128, 696)]
    try:
        loc.run_dev(bufs[0].ptr, 3, [0, len(scan)], bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr)
        c.synchronize()
        return bufs[2].download(np.float64, 7), bufs[3].download(L.RESULT_DTYPE, 1), bufs[4].download(np.uint8, 696)
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("plain", [0, 1], ids=["planes", "plain"])
def test_localising_in_a_cropped_surfel_map_equals_a_map_built_from_the_kept_points(plain):
    """run on map M cropped to box B == run on a fresh map of only those points of the same clouds whose voxel the rule keeps (per
    voxel the same sums and counts; `first` differs and is not read)"""
    c = ctx()
    scans, poses = L.drive("lot")
    n_map, per = 4, L.H * L.W
    pts, off = np.ascontiguousarray(scans[:n_map].reshape(-1, 3)), [i * per for i in range(n_map + 1)]
    leaf = 0.5
    centre = np.concatenate([UNIT_Q, poses[n_map][4:7]])
    lo, hi = [-12.0, -9.0, -30.0], [14.0, 11.0, 30.0]
    _, flo, fhi = X.crop_bounds(centre, lo, hi, leaf)
    kept_pts, kept_off = [], [0]
    for i in range(n_map):
        what, _, key, _, _ = SM.point_terms(scans[i], poses[i], leaf, 0.5, 120.0)
        keep = np.array([w == CM.USED and X.keeps(k, flo, fhi) for w, k in zip(what, key)])
        kept_pts.append(scans[i][keep])
        kept_off.append(kept_off[-1] + int(keep.sum()))
    assert 0 < kept_off[-1] < off[-1]
    params = capi.SurfelMapParams(leaf, 0.5, 120.0)
    m, fresh, whole = c.surfel_map(params, 1 << 15), c.surfel_map(params, 1 << 15), c.surfel_map(params, 1 << 15)
    locs = [x.localizer(1, per) for x in (m, fresh, whole)]
    try:
        with option("NO_LOCALIZE_PLANES", plain):
            dev_add(m, pts, off, poses[:n_map])
            dev_add(whole, pts, off, poses[:n_map])
            dev_add(fresh, np.concatenate(kept_pts), kept_off, poses[:n_map])
            _run(locs[0], np.ascontiguousarray(scans[n_map]), poses[n_map])  # a run before the crop: the plane cache holds the uncropped map
            counts = dev_crop(m, lo, hi, centre)
            assert counts[0] == fresh.stats()["voxels"] and counts[1] > 100 and counts[2] == 0
            start = L.displaced(poses[n_map], 0.1, 0.5, seed=3)
            scan = np.ascontiguousarray(scans[n_map])
            got, want, uncropped = _run(locs[0], scan, start), _run(locs[1], scan, start), _run(locs[2], scan, start)
        for g, w, name in zip(got, want, ("pose", "result", "information")):
            assert CM.same_bytes(g, w), name
        assert got[1]["n_rows"][0] > 500 and got[1]["termination"][0] in (L.CONVERGED, L.MAX_ITERATIONS)
        assert not CM.same_bytes(got[1], uncropped[1])  # (the crop took planes the scan used in the whole map)
    finally:
        for x in locs + [m, fresh, whole]:
            x.close()


# ---- 9. the loop without a synchronise ----------------------------------------------------------------------------------------------------
def test_localise_add_crop_three_times_without_a_synchronise_equals_the_host_forms():
    c = ctx()
    scans, poses = L.drive("lot")
    n_map, n_loop, per = 4, 3, L.H * L.W
    params = capi.SurfelMapParams(0.5, 0.5, 120.0)
    lo, hi = [-15.0] * 3, [15.0] * 3
    starts = np.stack([L.displaced(poses[n_map + i], 0.1, 0.5, seed=i) for i in range(n_loop)])
    dev, host = c.surfel_map(params, 1 << 15), c.surfel_map(params, 1 << 15)
    loc_dev, loc_host = dev.localizer(1, per), host.localizer(1, per)
    flat = np.ascontiguousarray(scans[:n_map + n_loop].reshape(-1, 3))
    bufs = [c.alloc(flat.nbytes).upload(flat), c.alloc(n_map * 56).upload(np.ascontiguousarray(poses[:n_map])), c.alloc(starts.nbytes).upload(starts)]
    bufs += [c.alloc(n).upload(np.full(n, POISON, dtype=np.uint8)) for n in (n_loop * 56, n_loop * 128, n_loop * 16)]
    d_pts, d_map_poses, d_start, d_out, d_res, d_counts = bufs
    try:
        # the host forms, a synchronise behind each
        for i in range(n_map):
            host.add_cloud(scans[i], poses[i])
        want_poses, want_counts = [], []
        for i in range(n_loop):
            pose, _, _ = loc_host.run(scans[n_map + i], starts[i], information=False)
            host.add_cloud(scans[n_map + i], pose)
            want_counts.append(host.crop(lo, hi, pose[4:7]))
            want_poses.append(pose)
        want = host.emit()
        # the device forms: nothing waits before the end
        c.synchronize()
        dev.add_clouds_dev(d_pts.ptr, 3, [i * per for i in range(n_map + 1)], d_map_poses.ptr)
        for i in range(n_loop):
            scan = d_pts.ptr + (n_map + i) * per * 24
            loc_dev.run_dev(scan, 3, [0, per], d_start.ptr + i * 56, d_out.ptr + i * 56, d_res.ptr + i * 128)
            dev.add_clouds_dev(scan, 3, [0, per], d_out.ptr + i * 56)
            dev.crop_dev(lo, hi, d_out.ptr + i * 56, d_counts.ptr + i * 16)
        c.synchronize()
        got_poses, got_counts = d_out.download(np.float64, n_loop * 7).reshape(n_loop, 7), d_counts.download(np.uint32, n_loop * 4).reshape(n_loop, 4)
        got = dev.emit()
        assert CM.same_bytes(got_poses, np.stack(want_poses))
        assert got_counts.tolist() == [[k, r, 0, 0] for k, r in want_counts]
        assert sum(r for _, r in want_counts) > 100 and all(k > 100 for k, _ in want_counts)
        SM.assert_emit_equal(got, want, "the loop")
        assert stats_of("surfel", dev.stats()) == stats_of("surfel", host.stats())
    finally:
        for b in bufs:
            b.free()
        for x in (loc_dev, loc_host, dev, host):
            x.close()
