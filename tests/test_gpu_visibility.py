"""GPU: the map cleaning (include/loamx.h, "map cleaning"; loam_amd/csrc/visibility_kernels.hip) against the numpy model of
tests/visibility_common.py, by equality of bytes: votes, the census, the dynamic flags, the kept points and their order. Every
output is poisoned before the call and what lies past it must stay poison. The form that reads squared ranges a first launch
wrote and the form that reads the scans' points (context option NO_VISIBILITY_RANGES) must agree with each other as well as with
the model."""
import ctypes as C
import functools

import numpy as np
import pytest

import cloudmap_common as CM
import organize_common as O
import visibility_common as V
from gpu_common import ctx, option
from loam_amd import capi
from map_common import small_pose

pytestmark = pytest.mark.gpu

POISON = 0xA5
POISON_U32 = np.uint32(0xA5A5A5A5)
FAN = (15.0, -15.0)
FORMS = (0, 1)
IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
GUARD = 3  # records behind every output that must stay poison


def make_layout(H, W, fan=FAN, clockwise=False):
    return ctx().scan_layout(capi.LidarParams(H, W, 1.0, 120.0), capi.OrganizeParams(elevations=O.fan_elevations(H, fan), clockwise=clockwise))


def to_capi(p):
    return capi.VisibilityParams(**(p or V.Params()).items())


def poisoned(c, nbytes):
    b = c.alloc(max(nbytes, 8))
    b.upload(np.full(b.nbytes, POISON, dtype=np.uint8))
    return b


def run_votes(layout, pts, scans, poses, params=None, accumulate=False, start=None):
    """votes_dev on uploaded copies into a poisoned (or `start`) buffer -> (votes (n,), census); nothing past n may be written"""
    c = ctx()
    pts, scans, poses = np.ascontiguousarray(pts, dtype=np.float64), np.ascontiguousarray(scans), np.ascontiguousarray(poses, dtype=np.float64)
    n, ns = len(pts), len(scans)
    assert scans.dtype in (np.float32, np.float64) and (ns == 0 or scans[0].size == layout.cells * 3)
    bufs = [c.alloc(max(pts.nbytes, 8)), c.alloc(max(scans.nbytes, 8)), c.alloc(max(poses.nbytes, 8)), poisoned(c, (n + GUARD) * 16)]
    try:
        for b, a in zip(bufs, (pts, scans, poses)):
            if a.size:
                b.upload(a)
        if start is not None:
            bufs[3].upload(np.ascontiguousarray(start))
        c.visibility_votes_dev(layout, bufs[0].ptr, pts.shape[1], n, bufs[1].ptr, ns, bufs[2].ptr, bufs[3].ptr, to_capi(params), accumulate,
                               f32=scans.dtype == np.float32)
        census = c.last_visibility_census()
        words = bufs[3].download(np.uint32, (n + GUARD) * 4)
    finally:
        for b in bufs:
            b.free()
    assert (words[n * 4:] == POISON_U32).all(), "votes written past n_points"
    return words[:n * 4].copy().view(V.VOTES_DTYPE), census


def tally(verdict):
    """(n_scans, n) verdicts -> (n,) votes"""
    out = np.zeros(verdict.shape[1], dtype=V.VOTES_DTYPE)
    for k, name in enumerate(V.FIELDS):
        out[name] = (verdict == k).sum(axis=0)
    return out


def model_verdicts(layout, pts, scans, poses, params=None, clockwise=False):
    """((n_scans, n) verdicts, (n_scans, n) places) by the model on the library's own tables"""
    col, tan = layout.tables()
    H, W = layout.scan_lines, layout.points_per_line
    out = [V.verdicts(pts, scans[s], poses[s], H, W, col, tan, clockwise, params) for s in range(len(scans))]
    n = len(pts)
    return (np.array([o[0] for o in out]).reshape(len(scans), n), np.array([o[1] for o in out]).reshape(len(scans), n))


def check_votes(layout, pts, scans, poses, verdict, place, params=None, what=""):
    """both forms against the model's verdicts of exactly these points and scans"""
    want = tally(verdict)
    for form in FORMS:
        with option("NO_VISIBILITY_RANGES", 1 - form):
            got, census = run_votes(layout, pts, scans, poses, params)
        assert V.same_bytes(got, want), (what, form, np.flatnonzero(got != want)[:5])
        assert census == (form, -(-len(scans) // V.SCAN_CHUNK), int((place >= 1).sum()), int((place == 2).sum())), (what, form, census)
        assert census.projected_pairs == sum(int(want[f].sum()) for f in V.FIELDS)
    return want


def scene(rng, H, W, n_points, n_scans, dtype, stride=3):
    """map points around a handful of tilted sensor poses, the non-finite ones first, and a holey scan per pose"""
    poses = np.stack([small_pose(rng, angle=0.1, shift=2.0) for _ in range(n_scans)])
    k = min(3, n_scans - 1)
    if k > 0:
        poses[1:1 + k, :4] *= np.array([[1.2], [0.7], [1.0]])[:k]  # quaternions are used as given
    pts = np.full((n_points, stride), np.nan)  # (the scalars behind z are never read)
    pts[:, :3] = V.cloud(rng, n_points)
    pts[:4, :3] = [[np.nan, 1, 1], [poses[0, 4], poses[0, 5], poses[0, 6]], [1, -np.inf, 1], [1e200, 1e200, 1]][:min(4, n_points)]
    scans = np.stack([V.shell_scan(rng, H, W, dtype=dtype) for _ in range(n_scans)])
    if n_scans > 1:
        scans[1] = 0.0  # a scan without a single return: EMPTY wherever a point has a cell
    return pts, scans, poses


# ---- 1. point and scan counts, layouts, scalar types, strides ----------------------------------------------------------------------
N_POINTS = (0, 1, 255, 256, 257, 1000)
N_SCANS = (0, 1, 2, 7, V.SCAN_CHUNK + 1)


@pytest.mark.parametrize("H,W,dtype,stride", [(2, 4, np.float64, 3), (2, 4, np.float32, 5), (16, 256, np.float64, 3), (16, 256, np.float32, 5),
                                               (16, 256, np.float64, 5), (16, 256, np.float32, 3), (5, 37, np.float64, 3), (5, 37, np.float32, 5),
                                               (2, 4096, np.float32, 3)])  # (2 x 4096: tables too large for LDS, read where the layout keeps them)
def test_votes_and_census_for_every_count_of_points_and_scans(H, W, dtype, stride):
    rng = np.random.default_rng([41, H, W])
    layout = make_layout(H, W)
    try:
        pts, scans, poses = scene(rng, H, W, max(N_POINTS), max(N_SCANS), dtype, stride)
        verdict, place = model_verdicts(layout, pts, scans, poses)
        assert all((verdict == k).any() for k in range(5)), np.bincount(verdict.ravel(), minlength=5)
        for n in N_POINTS:
            for ns in N_SCANS:
                check_votes(layout, pts[:n], scans[:ns], poses[:ns], verdict[:ns, :n], place[:ns, :n], None, (n, ns))
    finally:
        layout.close()


def test_a_clockwise_layout_and_tilted_fans():
    rng = np.random.default_rng(42)
    layout = make_layout(6, 48, fan=(2.0, -24.8), clockwise=True)
    try:
        pts, scans, poses = scene(rng, 6, 48, 500, 5, np.float32)
        verdict, place = model_verdicts(layout, pts, scans, poses, clockwise=True)
        assert (place == 2).sum() > 200
        check_votes(layout, pts, scans, poses, verdict, place)
    finally:
        layout.close()


# ---- 2. windows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wl,wc", [(0, 0), (1, 1), (3, 3), (0, 3), (2, 0)])
def test_every_window_on_a_wide_scan_and_on_four_columns(wl, wc):
    rng = np.random.default_rng([43, wl, wc])
    p = V.Params(window_lines=wl, window_cols=wc)
    for H, W in ((3, 4), (16, 256), (1, 1), (3, 2)):
        layout = ctx().scan_layout(capi.LidarParams(H, W, 1.0, 120.0)) if H == 1 else make_layout(H, W)
        try:
            pts, scans, poses = scene(rng, H, W, 600, 3, np.float64)
            verdict, place = model_verdicts(layout, pts, scans, poses, p)
            check_votes(layout, pts, scans, poses, verdict, place, p, (H, W))
        finally:
            layout.close()


# ---- 3. the five verdicts by hand, at the clipped lines and the seam ---------------------------------------------------------------
def test_a_hand_built_scan_for_each_verdict_on_every_cell():
    H, W = 4, 8
    layout = make_layout(H, W)
    try:
        el, az = O.fan_elevations(H, FAN), 2.0 * np.pi * np.arange(W) / W
        d = np.stack([np.cos(el)[:, None] * np.cos(az)[None, :], np.cos(el)[:, None] * np.sin(az)[None, :], np.broadcast_to(np.sin(el)[:, None], (H, W))], -1)
        d = d.reshape(-1, 3)
        pts = 10.0 * d  # one point per cell: lines 0 and H - 1 have clipped windows, columns 0 and W - 1 windows across the seam
        assert np.array_equal(O.classify(pts, *layout.tables())[0], np.arange(H * W))
        holes = 50.0 * d
        holes[::3], holes[1::3, 2] = 0.0, np.nan  # every window still holds a far return: THROUGH
        scans = np.stack([np.zeros_like(d), 10.0 * d, 50.0 * d, 4.0 * d, holes])  # EMPTY, AGREE, THROUGH, OCCLUDED, THROUGH
        poses = np.tile(IDENTITY, (len(scans), 1))
        verdict, place = model_verdicts(layout, pts, scans, poses)
        want = check_votes(layout, pts, scans, poses, verdict, place)
        assert (want["empty"] == 1).all() and (want["agree"] == 1).all() and (want["through"] == 2).all() and (want["occluded"] == 1).all()
        # NONE: the same pairs with the points beyond max_range vote nowhere and count nowhere
        p = V.Params(max_range=5.0)
        verdict, place = model_verdicts(layout, pts, scans, poses, p)
        want = check_votes(layout, pts, scans, poses, verdict, place, p)
        assert (verdict == V.NONE).all() and not want.view(np.uint32).any()
        # one near return in the line below turns THROUGH into OCCLUDED; the own cell alone (window 0 / 0) still says THROUGH
        graze = 50.0 * d
        graze[:W] = 4.0 * d[:W]
        for p, field in ((V.Params(), "occluded"), (V.Params(window_lines=0, window_cols=0), "through")):
            verdict, place = model_verdicts(layout, pts[W:2 * W], graze[None], poses[:1], p)
            want = check_votes(layout, pts[W:2 * W], graze[None], poses[:1], verdict, place, p)
            assert (want[field] == 1).all()
    finally:
        layout.close()


# ---- 4. accumulate ---------------------------------------------------------------------------------------------------------------
def test_votes_over_a_then_b_equal_votes_over_both_and_the_sum_of_the_singles():
    rng = np.random.default_rng(44)
    H, W = 5, 37
    layout = make_layout(H, W)
    try:
        pts, scans, poses = scene(rng, H, W, 700, 7, np.float32)
        verdict, place = model_verdicts(layout, pts, scans, poses)
        want = tally(verdict)
        for form in FORMS:
            with option("NO_VISIBILITY_RANGES", 1 - form):
                a, census = run_votes(layout, pts, scans[:3], poses[:3])
                assert census.projected_pairs == int((place[:3] == 2).sum())
                ab, census = run_votes(layout, pts, scans[3:], poses[3:], accumulate=True, start=np.concatenate([a.view(np.uint32), np.full(4 * GUARD, POISON_U32)]))
                assert V.same_bytes(ab, want) and census.projected_pairs == int((place[3:] == 2).sum())  # (the census is the call's alone)
                singles = np.zeros(len(pts), dtype=V.VOTES_DTYPE)
                for s in range(len(scans)):
                    singles, _ = run_votes(layout, pts, scans[s:s + 1], poses[s:s + 1], accumulate=True,
                                           start=np.concatenate([singles.view(np.uint32), np.full(4 * GUARD, POISON_U32)]))
                assert V.same_bytes(singles, want)
                # no scans: accumulate keeps what is there, a plain call zeroes it
                kept, census = run_votes(layout, pts, scans[:0], poses[:0], accumulate=True, start=np.concatenate([a.view(np.uint32), np.full(4 * GUARD, POISON_U32)]))
                assert V.same_bytes(kept, a) and census == (form, 0, 0, 0)
                zeroed, _ = run_votes(layout, pts, scans[:0], poses[:0])
                assert not zeroed.view(np.uint32).any()
    finally:
        layout.close()


def test_the_host_form_equals_the_device_form():
    rng = np.random.default_rng(45)
    H, W = 5, 37
    layout = make_layout(H, W)
    try:
        for dtype in (np.float64, np.float32):
            pts, scans, poses = scene(rng, H, W, 300, 4, dtype, stride=4)
            want = tally(model_verdicts(layout, pts, scans, poses)[0])
            assert V.same_bytes(ctx().visibility_votes(pts, scans, poses, layout), want)
        assert len(ctx().visibility_votes(np.empty((0, 3)), scans, poses, layout)) == 0
        assert not ctx().visibility_votes(pts, scans[:0], poses[:0], layout).view(np.uint32).any()
        with pytest.raises(ValueError):
            ctx().visibility_votes(pts, scans, poses[:2], layout)
    finally:
        layout.close()


# ---- 5. the filter ---------------------------------------------------------------------------------------------------------------
def run_filter(votes, params=None, pts=None, capacity=0, with_dynamic=True, with_xyz=True, with_index=True):
    """filter_dev into poisoned buffers -> (dynamic or None, xyz or None, index or None, n); checks what must stay poison"""
    c = ctx()
    n = len(votes)
    stride = 3 if pts is None else pts.shape[1]
    room = capacity + GUARD
    bufs = [c.alloc(max(votes.nbytes, 8)), c.alloc(max(0 if pts is None else pts.nbytes, 8)), poisoned(c, n + GUARD), poisoned(c, room * 24),
            poisoned(c, room * 4), poisoned(c, 16)]
    try:
        if n:
            bufs[0].upload(np.ascontiguousarray(votes))
        if pts is not None and pts.size:
            bufs[1].upload(np.ascontiguousarray(pts, dtype=np.float64))
        c.visibility_filter_dev(bufs[0].ptr, n, bufs[5].ptr, to_capi(params), bufs[1].ptr if pts is not None else 0, stride,
                                bufs[2].ptr if with_dynamic else 0, bufs[3].ptr if with_xyz else 0, bufs[4].ptr if with_index else 0, capacity)
        c.synchronize()
        dyn, xyz = bufs[2].download(np.uint8, n + GUARD), bufs[3].download(np.float64, room * 3).reshape(room, 3)
        index, n_words = bufs[4].download(np.uint32, room), bufs[5].download(np.uint32, 4)
    finally:
        for b in bufs:
            b.free()
    kept = int(n_words[0])
    assert (n_words[1:] == POISON_U32).all()
    k = min(kept, capacity)
    writes_xyz = with_xyz and pts is not None
    assert (dyn[n if with_dynamic else 0:] == POISON).all(), "flags written past n_points"
    assert (xyz[k if writes_xyz else 0:].view(np.uint8) == POISON).all(), "points written past min(n, capacity)"
    assert (index[k if with_index else 0:] == POISON_U32).all(), "indices written past min(n, capacity)"
    return dyn[:n].copy() if with_dynamic else None, xyz[:k].copy() if writes_xyz else None, index[:k].copy() if with_index else None, kept


def check_filter(votes, params, pts, capacity, **kw):
    got = run_filter(votes, params, pts, capacity, **kw)
    dyn, xyz, keep, n = V.filter_static(votes, params, pts, capacity)
    assert got[3] == n, (got[3], n)
    assert got[0] is None or V.same_bytes(got[0], dyn)
    assert got[1] is None or V.same_bytes(got[1], xyz)
    assert got[2] is None or V.same_bytes(got[2], keep)
    return n


def test_the_filter_at_the_edges_of_the_rule_with_every_capacity_and_every_missing_output():
    rng = np.random.default_rng(46)
    edges = [(t, a, o, 7) for t in (0, 1, 2, 3, 4, 5, 0xFFFFFFFF) for a in (0, 1, 2, 3, 4, 0xFFFFFFFF) for o in (0, 9)]
    votes = np.array(edges + [tuple(r) for r in rng.integers(0, 6, (1000 - len(edges), 4))], dtype=V.VOTES_DTYPE)
    pts = rng.normal(size=(len(votes), 5))
    for p in (V.Params(), V.Params(min_through=0), V.Params(min_through=3, through_ratio=0.5), V.Params(through_ratio=1.5), V.Params(through_ratio=0.0),
              V.Params(min_through=0xFFFFFFFF), V.Params(through_ratio=1.0 / 3.0)):
        n = check_filter(votes, p, pts, len(votes))
        assert p.min_through == 0xFFFFFFFF or 0 < n < len(votes) or p.through_ratio == 0.0
    n = V.filter_static(votes)[3]
    for capacity in (0, 1, n // 2, n - 1, n, n + 1):
        check_filter(votes, None, pts, capacity)
    for n_points in (0, 1, 255, 256, 257):
        check_filter(votes[:n_points], None, pts[:n_points], n_points)
    for with_dynamic in (False, True):
        for with_xyz in (False, True):
            for with_index in (False, True):
                if not with_xyz:  # (without the points' output the points themselves may be missing as well)
                    check_filter(votes, None, None, 100, with_dynamic=with_dynamic, with_xyz=False, with_index=with_index)
                    check_filter(votes, None, pts, 0, with_dynamic=with_dynamic, with_xyz=False, with_index=with_index)
                else:
                    check_filter(votes, None, pts, 100, with_dynamic=with_dynamic, with_index=with_index)
    # a pointer for the points' output without the points: nothing to read them from, nothing is written there
    got = run_filter(votes, None, None, 100)
    assert got[1] is None and V.same_bytes(got[2], V.filter_static(votes, None, None, 100)[2])


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_outputs_untouched():
    c = ctx()
    lib = c.lib
    nan, inf = float("nan"), float("inf")
    layout = make_layout(2, 4)
    bufs = [c.alloc(1024), c.alloc(2 * 4 * 3 * 8 * 2), c.alloc(7 * 8 * 2), poisoned(c, 1024), poisoned(c, 1024), poisoned(c, 1024), poisoned(c, 1024)]
    d_pts, d_scans, d_poses, d_votes, d_dyn, d_xyz, d_n = (b.ptr for b in bufs)
    try:
        for b in bufs[:3]:
            b.upload(np.zeros(b.nbytes, dtype=np.uint8))

        def votes(layout_h=layout.h, pts=d_pts, stride=3, n=8, scans=d_scans, ns=2, poses=d_poses, params="default", out=d_votes, f32=False, **kw):
            st = capi.VisibilityParams(**kw).struct()
            fn = lib.loamx_visibility_votes_dev_f32 if f32 else lib.loamx_visibility_votes_dev
            return fn(c.h, layout_h, pts, stride, n, scans, ns, poses, C.byref(st) if params == "default" else None, 0, out)

        def filt(votes_p=d_votes, n=8, params="default", pts=d_pts, stride=3, dyn=d_dyn, xyz=d_xyz, index=None, capacity=8, n_out=d_n, **kw):
            st = capi.VisibilityParams(**kw).struct()
            return lib.loamx_visibility_filter_dev(c.h, votes_p, n, C.byref(st) if params == "default" else None, pts, stride, dyn, xyz, index, capacity, n_out)

        bad, unsupported = capi.ERR_BAD_PARAM, capi.ERR_UNSUPPORTED
        for f32 in (False, True):
            assert votes(layout_h=None, f32=f32) == bad and votes(params=None, f32=f32) == bad and votes(out=None, f32=f32) == bad
            assert votes(pts=None, f32=f32) == bad and votes(scans=None, f32=f32) == bad and votes(poses=None, f32=f32) == bad
            assert votes(stride=2, f32=f32) == bad and votes(stride=0, f32=f32) == bad
            assert votes(n=1 << 32, f32=f32) == unsupported and votes(ns=1 << 31, f32=f32) == unsupported
        assert lib.loamx_visibility_votes_dev(None, layout.h, d_pts, 3, 8, d_scans, 2, d_poses, C.byref(capi.VisibilityParams().struct()), 0, d_votes) == bad
        param_cases = [dict(min_range=-0.5), dict(min_range=10.0, max_range=9.0), dict(margin=-1e-9), dict(margin_rel=-1.0), dict(through_ratio=-0.1)]
        param_cases += [{name: v} for name in ("min_range", "max_range", "margin", "margin_rel", "through_ratio") for v in (nan, inf, -inf)]
        for kw in param_cases:
            assert votes(**kw) == bad and filt(**kw) == bad, kw
        for kw in (dict(window_lines=4), dict(window_cols=4), dict(window_lines=0xFFFFFFFF)):
            assert votes(**kw) == unsupported and filt(**kw) == unsupported, kw
        assert filt(n_out=None) == bad and filt(votes_p=None) == bad and filt(params=None) == bad and filt(stride=2) == bad
        assert filt(xyz=None) == bad and filt(n=1 << 32) == unsupported
        assert lib.loamx_visibility_filter_dev(None, d_votes, 8, C.byref(capi.VisibilityParams().struct()), None, 3, None, None, None, 0, d_n) == bad
        c.synchronize()
        for b in bufs[3:]:
            assert (b.download(np.uint8, b.nbytes) == POISON).all(), "a refused call wrote to an output"
        # what is allowed: the limits themselves, no points or no scans with null pointers, no xyz output without a capacity
        assert votes(window_lines=3, window_cols=3, min_range=0.0, max_range=0.0, margin=0.0, margin_rel=0.0, through_ratio=0.0) == capi.OK
        assert votes(pts=None, n=0, out=None) == capi.OK and votes(scans=None, poses=None, ns=0) == capi.OK
        assert filt(xyz=None, capacity=0) == capi.OK and filt(votes_p=None, n=0, pts=None) == capi.OK
        c.synchronize()
    finally:
        layout.close()
        for b in bufs:
            b.free()


def test_the_census_before_any_votes_call_is_refused():
    c = capi.Context(0)
    try:
        with pytest.raises(capi.LoamxError) as e:
            c.last_visibility_census()
        assert e.value.status == capi.ERR_BAD_PARAM
    finally:
        c.close()


# ---- 7. the chain on the drive ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def drive_model():
    """the drive of visibility_common with its scans shuffled into unordered clouds, and everything the chain should produce"""
    d = V.drive()
    rng = np.random.default_rng(47)
    clouds = np.stack([s[rng.permutation(d["H"] * d["W"])] for s in d["scans"]])
    return d, clouds


def test_the_chain_from_unordered_clouds_to_the_cleaned_map_without_a_synchronise():
    c = ctx()
    d, clouds = drive_model()
    H, W, n, leaf = d["H"], d["W"], len(d["scans"]), d["leaf"]
    layout = make_layout(H, W, fan=V.S.FANS["lot"])
    col, tan = layout.tables()
    # the model: organise, map, votes, filter
    scans = np.stack([O.organize(cl, H, W, col, tan)[0] for cl in clouds])
    model = CM.CloudMapModel(leaf, 0.5, 120.0)
    offsets = np.arange(n + 1) * (H * W)
    model.add(scans.reshape(-1, 3), offsets, d["poses"])
    points = model.emit()[0]
    n_vox = len(points)
    want_votes, in_range, projected = V.votes(points, scans, d["poses"], H, W, col, tan)
    want_dyn, want_xyz, want_keep, want_n = V.filter_static(want_votes, None, points)
    assert 0 < want_dyn.sum() < n_vox // 20 and in_range > projected > 10 * n_vox

    cmap = c.cloud_map(capi.CloudMapParams(leaf, 0.5, 120.0), 1 << 15)
    bufs = [c.alloc(clouds.nbytes), c.alloc(clouds.nbytes), c.alloc(d["poses"].nbytes), poisoned(c, (1 << 15) * 24), poisoned(c, 16),
            poisoned(c, n_vox * 16), poisoned(c, n_vox), poisoned(c, n_vox * 24), poisoned(c, n_vox * 4), poisoned(c, 16)]
    d_clouds, d_scans, d_poses, d_xyz, d_n, d_votes, d_dyn, d_static, d_index, d_n_static = bufs
    try:
        for form in FORMS:
            with option("NO_VISIBILITY_RANGES", 1 - form):
                d_clouds.upload(clouds), d_poses.upload(d["poses"])
                cmap.clear()
                c.organize_clouds_dev(layout, d_clouds.ptr, 3, offsets, d_scans.ptr, f32=True)
                cmap.add_clouds_dev(d_scans.ptr, 3, offsets, d_poses.ptr, f32=True)
                cmap.emit_dev(d_xyz.ptr, 1 << 15, d_n.ptr)
                c.visibility_votes_dev(layout, d_xyz.ptr, 3, n_vox, d_scans.ptr, n, d_poses.ptr, d_votes.ptr, f32=True)
                c.visibility_filter_dev(d_votes.ptr, n_vox, d_n_static.ptr, None, d_xyz.ptr, 3, d_dyn.ptr, d_static.ptr, d_index.ptr, n_vox)
                c.synchronize()  # (the first one)
            assert int(d_n.download(np.uint32, 1)[0]) == n_vox
            assert V.same_bytes(d_xyz.download(np.float64, n_vox * 3).reshape(-1, 3), points)
            assert V.same_bytes(d_votes.download(np.uint32, n_vox * 4).view(V.VOTES_DTYPE), want_votes), form
            assert c.last_visibility_census() == (form, 1, in_range, projected)
            assert int(d_n_static.download(np.uint32, 1)[0]) == want_n
            assert V.same_bytes(d_dyn.download(np.uint8, n_vox), want_dyn)
            assert V.same_bytes(d_static.download(np.float64, want_n * 3).reshape(-1, 3), want_xyz)
            assert V.same_bytes(d_index.download(np.uint32, want_n), want_keep)
    finally:
        cmap.close(), layout.close()
        for b in bufs:
            b.free()
