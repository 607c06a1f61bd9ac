"""GPU: the occupancy ray cast (include/loamx.h, "occupancy ray casting"; loam_amd/csrc/raycast_kernels.hip) against the Python
model of tests/raycast_common.py, by equality of bytes: the records of cast segments, the scans, ranges and records of rendered
scans, and the census. Outputs are poisoned before every call. The plain form (the default) and the combining one (context option
RAYCAST_COMBINE) must leave the same bytes; `probes` tells them apart."""
import ctypes as C

import numpy as np
import pytest

import cloudmap_common as CM
import localize_common as L
import occupancy_common as OM
import raycast_common as M
from gpu_common import ctx, option
from loam_amd import capi

pytestmark = pytest.mark.gpu

POISON = 0xA5
PAD = 3  # entries behind every output that must stay poison
FORMS = ("combined", "plain")


def form(name):
    return option("RAYCAST_COMBINE", 1 if name == "combined" else 0)


def _poisoned(c, nbytes):
    return c.alloc(nbytes).upload(np.full(nbytes, POISON, dtype=np.uint8))


def _take(buf, dtype, n, per=1):
    """the first n entries of a poisoned buffer of n + PAD, after checking that nothing behind them was written"""
    raw = buf.download(np.uint8, (n + PAD) * per * np.dtype(dtype).itemsize)
    used = n * per * np.dtype(dtype).itemsize
    assert (raw[used:] == POISON).all(), "written past the end"
    return raw[:used].view(dtype).copy()


def dev_cast(m, origins, ends, params=None, stride=3):
    """(records, census) of the device form on uploaded segments, (n, stride) each"""
    c = m.ctx
    o, e = np.ascontiguousarray(origins, dtype=np.float64), np.ascontiguousarray(ends, dtype=np.float64)
    n = len(o)
    bufs = [c.alloc(max(o.nbytes, 8)), c.alloc(max(e.nbytes, 8)), _poisoned(c, (n + PAD) * 40)]
    try:
        if n:
            bufs[0].upload(o), bufs[1].upload(e)
        m.cast_rays_dev(bufs[0].ptr, bufs[1].ptr, stride, n, bufs[2].ptr, capi.RaycastParams(**(params or {})))
        c.synchronize()
        return _take(bufs[2], capi.RAY_RECORD_DTYPE, n), c.last_raycast_census()
    finally:
        for b in bufs:
            b.free()


def dev_render(m, dirs, poses, max_range, params=None, want=(True, True, True)):
    """(scans, ranges, records, census) of the device form; an output that is not wanted is passed as NULL and comes back None"""
    c = m.ctx
    d, p = np.ascontiguousarray(dirs, dtype=np.float64), np.ascontiguousarray(poses, dtype=np.float64)
    n = len(d) * len(p)
    bufs = [c.alloc(max(d.nbytes, 8)).upload(d), c.alloc(max(p.nbytes, 8)).upload(p), _poisoned(c, (n + PAD) * 24), _poisoned(c, (n + PAD) * 8),
            _poisoned(c, (n + PAD) * 40)]
    try:
        m.render_scans_dev(bufs[0].ptr, len(d), bufs[1].ptr, len(p), max_range, capi.RaycastParams(**(params or {})),
                           *[b.ptr if w else 0 for b, w in zip(bufs[2:], want)])
        c.synchronize()
        shape = (len(p), len(d))
        scans = _take(bufs[2], np.float64, n if want[0] else 0, 3)
        ranges = _take(bufs[3], np.float64, n if want[1] else 0)
        records = _take(bufs[4], capi.RAY_RECORD_DTYPE, n if want[2] else 0)
        return (scans.reshape(*shape, 3) if want[0] else None, ranges.reshape(shape) if want[1] else None,
                records.reshape(shape) if want[2] else None, c.last_raycast_census())
    finally:
        for b in bufs:
            b.free()


_hand = None


def hand():
    """(map, model): the hand-made map at leaf 0.5, added through add_cloud into 128 slots"""
    global _hand
    if _hand is None:
        m = ctx().occupancy_map(capi.OccupancyParams(**M.HAND_PARAMS), M.HAND_MAX_VOXELS)
        m.add_cloud(M.hand_cloud(), M.HAND_POSE)
        model = M.hand_model()
        OM.assert_stats_equal(m.stats(), model.stats(), "the hand-made map")
        _hand = (m, model, M.StateMap.of(model))
    return _hand


_model_cache = {}


def model_cast(key, o, e, states, P):
    if key not in _model_cache:
        _model_cache[key] = M.cast(o, e, M.LEAF, states, P)
    return _model_cache[key]


def check_cast(m, states, o, e, P, key, stride=3):
    """both forms against the model and against each other; the census of each"""
    want, census = model_cast(key, o, e, states, P)
    got = {}
    for f in FORMS:
        with form(f):
            oo, ee = (o, e) if stride == 3 else [np.concatenate([a, np.full((len(a), stride - 3), 1e300)], axis=1) for a in (o, e)]
            got[f], c = dev_cast(m, oo, ee, P, stride)
        assert M.same_bytes(got[f], want), (key, f, got[f][:8], want[:8])
        M.assert_census(c, census, f == "combined", (key, f))
        if f == "plain":
            assert int(c["probes"]) == int(c["visits"])
    assert got["combined"].tobytes() == got["plain"].tobytes()
    return want, census


CASES = M.ray_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_alone_under_every_variant_of_the_parameters(name):
    m, _, states = hand()
    for variant, P in M.PARAM_VARIANTS.items():
        check_cast(m, states, *CASES[name], P, (name, variant))


@pytest.mark.parametrize("variant", sorted(M.PARAM_VARIANTS))
def test_the_cases_mixed_inside_wavefronts(variant):
    m, _, states = hand()
    o, e = M.mixed_rays(257)
    want, census = check_cast(m, states, o, e, M.PARAM_VARIANTS[variant], ("mixed", variant))
    assert len(set(want["status"].tolist())) >= 4 and census["probes"][1] < census["probes"][0]


@pytest.mark.parametrize("n", M.RAY_COUNTS)
def test_ray_counts_around_a_wavefront_and_a_workgroup(n):
    m, _, states = hand()
    o, e = M.mixed_rays(n)
    assert len(o) == n
    check_cast(m, states, o, e, {}, ("count", n))
    check_cast(m, states, o, e, {}, ("count", n), stride=5)


def test_one_run_makes_one_look_up_per_trip_and_abab_none_fewer():
    m, _, states = hand()
    with form("combined"):
        _, c = dev_cast(m, *CASES["one_run"])
    assert int(c["probes"]) < int(c["visits"]) and int(c["probes"]) * 64 == int(c["visits"])
    with form("combined"):
        _, c = dev_cast(m, *CASES["alternating_abab"])
    assert int(c["probes"]) == int(c["visits"]) > 0


def test_the_empty_map_is_unknown_everywhere():
    c = ctx()
    m = c.occupancy_map(capi.OccupancyParams(**M.HAND_PARAMS), M.HAND_MAX_VOXELS)
    try:
        states = M.StateMap({})
        o, e = M.mixed_rays(130)
        for variant in ("default", "unknown_stops", "skip_start_1"):
            want, _ = check_cast(m, states, o, e, M.PARAM_VARIANTS[variant], ("empty", variant))
            assert M.HIT not in want["status"].tolist()
    finally:
        m.close()


def test_the_host_form_gives_the_same_records():
    m, _, states = hand()
    o, e = M.mixed_rays(65)
    want, census = model_cast(("count", 65), o, e, states, {})
    assert M.same_bytes(m.cast_rays(o, e), want)
    M.assert_census(m.ctx.last_raycast_census(), census, False)  # (the default form: every lane its own look-up)
    assert len(m.cast_rays(np.zeros((0, 3)), np.zeros((0, 3)))) == 0
    assert not any(int(v) for v in m.ctx.last_raycast_census().tolist())


def test_refusals_write_nothing():
    m, _, _ = hand()
    c = m.ctx
    o, e = M.mixed_rays(8)
    d_o, d_e, d_r = c.alloc(o.nbytes).upload(o), c.alloc(e.nbytes).upload(e), _poisoned(c, 8 * 40)
    other = capi.Context(0)
    foreign = other.occupancy_map(capi.OccupancyParams(**M.HAND_PARAMS), 64)
    P = capi.RaycastParams
    try:
        def refused(status, fn):
            with pytest.raises(capi.LoamxError) as err:
                fn()
            assert err.value.status == status, err.value
        bad, unsupported = capi.ERR_BAD_PARAM, capi.ERR_UNSUPPORTED
        refused(bad, lambda: m.cast_rays_dev(0, d_e.ptr, 3, 8, d_r.ptr))
        refused(bad, lambda: m.cast_rays_dev(d_o.ptr, 0, 3, 8, d_r.ptr))
        refused(bad, lambda: m.cast_rays_dev(d_o.ptr, d_e.ptr, 3, 8, 0))
        refused(bad, lambda: m.cast_rays_dev(d_o.ptr, d_e.ptr, 2, 8, d_r.ptr))
        refused(bad, lambda: m.cast_rays_dev(d_o.ptr, d_e.ptr, 3, 8, d_r.ptr, P(hit_at=2)))
        st = P().struct()  # a map of another context
        refused(bad, lambda: c._check(c.lib.loamx_occupancy_cast_rays(c.h, foreign._handle(), d_o.ptr, d_e.ptr, 3, 8, C.byref(st), d_r.ptr)))
        refused(unsupported, lambda: m.cast_rays_dev(d_o.ptr, d_e.ptr, 3, 8, d_r.ptr, P(max_steps=(1 << 22) + 1)))
        refused(unsupported, lambda: m.cast_rays_dev(d_o.ptr, d_e.ptr, 3, (1 << 31) + 1, d_r.ptr))
        refused(unsupported, lambda: m.cast_rays_dev(d_o.ptr, d_e.ptr, 1 << 32, 8, d_r.ptr))
        refused(bad, lambda: m.render_scans_dev(d_o.ptr, 8, d_e.ptr, 1, 0.0, None, d_r.ptr))
        refused(bad, lambda: m.render_scans_dev(d_o.ptr, 8, d_e.ptr, 1, np.inf, None, d_r.ptr))
        refused(bad, lambda: m.render_scans_dev(d_o.ptr, 8, d_e.ptr, 1, np.nan, None, d_r.ptr))
        refused(bad, lambda: m.render_scans_dev(0, 8, d_e.ptr, 1, 5.0, None, d_r.ptr))
        refused(bad, lambda: m.render_scans_dev(d_o.ptr, 8, 0, 1, 5.0, None, d_r.ptr))
        refused(unsupported, lambda: m.render_scans_dev(d_o.ptr, 1 << 16, d_e.ptr, (1 << 15) + 1, 5.0, None, d_r.ptr))
        m.cast_rays_dev(0, 0, 3, 0, 0)  # no ray: fine, nothing written
        m.render_scans_dev(0, 0, d_e.ptr, 4, 5.0)
        c.synchronize()
        assert (d_r.download(np.uint8, 8 * 40) == POISON).all()
        m.cast_rays_dev(d_o.ptr, d_e.ptr, 3, 8, d_r.ptr, P(max_steps=1 << 22))  # the largest cap is taken
        c.synchronize()
        assert (d_r.download(np.uint8, 8 * 40) != POISON).any()
        d_r.upload(np.full(8 * 40, POISON, dtype=np.uint8))
        refused(bad, lambda: m.cast_rays_dev(d_o.ptr, d_e.ptr, 3, 8, d_r.ptr, P(hit_at=7)))
        c.synchronize()
        assert (d_r.download(np.uint8, 8 * 40) == POISON).all()
    finally:
        foreign.close(), other.close()
        for b in (d_o, d_e, d_r):
            b.free()


# ---- rendered scans ---------------------------------------------------------------------------------------------------------------
RENDER_LEAF, RENDER_RANGE = 0.5, 40.0
_lot = None


def lot():
    """(map, model, states, scans, poses): two scans of the drive through the lot, added at their poses"""
    global _lot
    if _lot is None:
        scans, poses = L.drive("lot")
        scans, poses = scans[:2], np.ascontiguousarray(poses[:2])
        params = dict(leaf=RENDER_LEAF, min_range=0.5, max_range=80.0, end_margin=0.0, occ_ratio=0.0, min_hits=1)
        m, model = ctx().occupancy_map(capi.OccupancyParams(**params), 1 << 17), OM.OccupancyModel(**params)
        for s, p in zip(scans, poses):
            m.add_cloud(s, p)
            model.add(s, poses=p[None])
        OM.assert_stats_equal(m.stats(), model.stats(), "two scans of the lot")
        _lot = (m, model, M.StateMap.of(model), scans, poses)
    return _lot


def render_poses():
    _, _, _, _, poses = lot()
    q = np.array([0.05, -0.08, 0.3, 1.0])  # rotated about all three axes
    return np.stack([poses[0], np.concatenate([q / np.linalg.norm(q), poses[1][4:] + [0.3, -0.2, 0.1]])])


@pytest.mark.parametrize("hit_at", (capi.RAY_AT_ENTER, capi.RAY_AT_MIDDLE))
@pytest.mark.parametrize("shape", ((4, 64), (3, 70)))
def test_rendered_scans_equal_the_model(shape, hit_at):
    m, model, states, _, _ = lot()
    dirs = capi.beam_directions(*shape, capi.OrganizeParams(fov_bottom=np.radians(-12.0), fov_top=np.radians(6.0)))
    poses = render_poses()
    P = dict(hit_at=hit_at)
    want = M.render(dirs, poses, RENDER_RANGE, RENDER_LEAF, states, P)
    assert (want[2]["status"] == M.HIT).mean() > 0.3 and (want[1] > 1.0).sum() > 50
    got = {}
    for f in FORMS:
        with form(f):
            got[f] = dev_render(m, dirs, poses, RENDER_RANGE, P)
        for g, w, what in zip(got[f][:3], want[:3], ("scans", "ranges", "records")):
            assert M.same_bytes(g, w), (f, what)
        M.assert_census(got[f][3], want[3], f == "combined", f)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got["combined"][:3], got["plain"][:3]))
    assert int(got["combined"][3]["probes"]) < int(got["plain"][3]["probes"]) == int(got["plain"][3]["visits"])
    # each output NULL in turn: the others are the same bytes
    for k in range(3):
        wanted = tuple(i != k for i in range(3))
        part = dev_render(m, dirs, poses, RENDER_RANGE, P, wanted)
        assert part[k] is None and all(M.same_bytes(part[i], want[i]) for i in range(3) if i != k)
    # ... and the host form
    host = m.render_scans(dirs, poses, RENDER_RANGE, capi.RaycastParams(**P))
    assert all(M.same_bytes(h, w) for h, w in zip(host, want[:3]))


def test_a_pose_with_a_nan_gives_invalid_beams_and_a_zero_scan():
    m, model, states, _, _ = lot()
    dirs = capi.beam_directions(3, 70)
    poses = render_poses()
    poses[0, 2] = np.nan
    want = M.render(dirs, poses, RENDER_RANGE, RENDER_LEAF, states)
    scans, ranges, records, census = dev_render(m, dirs, poses, RENDER_RANGE)
    assert all(M.same_bytes(g, w) for g, w in zip((scans, ranges, records), want[:3]))
    assert (records["status"][0] == capi.RAY_INVALID).all() and not scans[0].any() and not np.signbit(scans[0]).any() and not ranges[0].any()
    assert int(census["invalid"]) == len(dirs) and (records["status"][1] == capi.RAY_HIT).any()


def test_every_ray_that_add_counted_as_a_hit_and_walked_is_hit_again():
    """Model-free: cloud_cell and the walk form floor(p' / leaf) by the same division, so the segment from a pose's t to pose.act(p)
    ends in p's own hit voxel, which is OCCUPIED under occ_ratio 0 and min_hits 1: the cast meets it or an obstacle before it."""
    m, model, _, scans, poses = lot()
    p = model.p
    lib = OM.hostcheck_lib()  # on the CPU first: the g++ build of the map's rule and its model agree on which rays those are
    n_hit = 0
    for scan, pose in zip(scans, poses):
        rays = OM.Rays(scan, pose, p["leaf"], p["min_range"], p["max_range"], p["end_margin"], p["clip_long"])
        pts = np.ascontiguousarray(scan, dtype=np.float64)
        kind, flags = np.zeros(len(pts), dtype=np.int32), np.zeros(len(pts), dtype=np.uint8)
        hit_key, steps = np.zeros(len(pts), dtype=np.uint64), np.zeros(len(pts), dtype=np.uint32)
        dp = C.POINTER(C.c_double)
        lib.hostcheck_occupancy_rays(pts.ctypes.data_as(dp), C.c_uint64(len(pts)), np.ascontiguousarray(pose).ctypes.data_as(dp), C.c_double(p["leaf"]),
                                     C.c_double(p["min_range"]), C.c_double(p["max_range"]), C.c_double(p["end_margin"]), C.c_uint32(p["clip_long"]),
                                     kind.ctypes.data_as(C.POINTER(C.c_int32)), flags.ctypes.data_as(C.POINTER(C.c_uint8)),
                                     hit_key.ctypes.data_as(C.POINTER(C.c_uint64)), steps.ctypes.data_as(C.POINTER(C.c_uint32)))
        sel = rays.has_hit & rays.walks
        assert np.array_equal((flags & 5) == 5, sel) and sel.sum() > 1000
        n_hit += int(rays.has_hit.sum())
        ends = CM.pose_act(pose, pts[sel])
        origins = np.broadcast_to(pose[4:7], ends.shape)
        for f in FORMS:
            with form(f):
                rec, census = dev_cast(m, origins, ends)
            assert (rec["status"] == capi.RAY_HIT).all(), (f, np.unique(rec["status"], return_counts=True))
            assert int(census["hit"]) == int(sel.sum()) and int(census["clear"]) == 0
    assert int(m.stats()["rays_hit"]) == n_hit
