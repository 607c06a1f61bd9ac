"""GPU parity on outdoor-shaped scans (tests/outdoor_scenes.py): a street canyon, a walled lot and an open field, ray-cast
at 64 x 1024 and 128 x 2048. Against the room of synth.h (0.5 m index cells, every beam returns, every range < 15 m)
these give 0.8-1.6 m cells, hundreds of points in a 3 x 3 x 3 block (the wide running numbers, the 5 x 5 x 5 rest kernel
and the cooperative leftover kernel), source features outside the target grid, no-return beams and returns beyond
max_range. Everything is checked against the oracle through the entry points users call; bars as everywhere in the suite:
index sequences identical, termination and iteration count identical, SE(3) within 1e-5, every ICF update within 1e-7,
neighbour lists equal in order and fits within check_kind's allowances."""
import contextlib
import functools

import numpy as np
import pytest

import outdoor_scenes as S
from gpu_common import ctx, option, pose_diff
from loam_amd import capi
from test_gpu_direct import check_kind

pytestmark = pytest.mark.gpu

SE3_TOL, UPDATE_TOL = 1e-5, 1e-7
IDENT = np.array([0, 0, 0, 1.0, 0, 0, 0])
EXTRACTION_OPTIONS = ["FORCE_TIE_REPLAY", "FORCE_SCAN_GIVEUP", "NO_FUSED_COMPACT", "NO_ROW_SELECT", "NO_MIS_SELECT",
                      "NO_SPLIT_CURV", "FUSED_ROWS"]
# the batch of test 3: 16 outdoor pairs, the three scenes interleaved
BATCH = [(S.SCENES[i % 3], 100 + i) for i in range(16)]


@functools.lru_cache(maxsize=None)
def outdoor_pair(name, seed, H=64, W=1024):
    return S.pair(name, seed, H, W)


@functools.lru_cache(maxsize=None)
def oracle_run(oracle, key, H, W, f32=False):
    """oracle features of (target, source) and its registration with per-iteration detail; key = (scene, seed) or
    ("room", seed) for the synth.h pair (seed, 0)"""
    if key[0] == "room":
        tgt, src = capi.synth_scan_host(key[1], 0, 0, H, W, 0.01), capi.synth_scan_host(key[1], 0, 1, H, W, 0.01)
    else:
        tgt, src = outdoor_pair(key[0], key[1], H, W)[:2]
    if f32:
        tgt, src = tgt.astype(np.float32).astype(np.float64), src.astype(np.float32).astype(np.float64)
    ea, pa = oracle.extract_features(tgt, H, W, 1.0, 120.0)
    eb, pb = oracle.extract_features(src, H, W, 1.0, 120.0)
    reg = oracle.register_features(src[eb], src[pb], tgt[ea], tgt[pa], want_info=True)
    return tgt, src, (ea, pa, eb, pb), reg


def check_record(oracle, rec, reg, where):
    po, to, io, _ = reg
    assert (int(rec["termination"]), int(rec["iterations"])) == (to, io), where
    rot, trans = pose_diff(oracle, po, rec["pose"])
    assert rot < SE3_TOL and trans < SE3_TOL, (where, rot, trans)


def check_detail(oracle, feats, tgt, src, reg, where):
    """loamx_register_features with detail: termination, iterations, every ICF update and the pose against the oracle"""
    ea, pa, eb, pb = feats
    po, to, io, info = reg
    pg, tg, ig, det = ctx().register_features(src[eb], src[pb], tgt[ea], tgt[pa], want_detail=True)
    assert (tg, ig) == (to, io), where
    assert len(det["iterations"]) == len(info) == io
    for i, (a, b) in enumerate(zip(info, det["iterations"])):
        assert (a.n_edge_assoc, a.n_plane_assoc) == (b["n_edge"], b["n_plane"]), (where, i)
        rot, trans = pose_diff(oracle, np.array(list(a.update)), b["estimate_update"])
        assert rot < UPDATE_TOL and trans < UPDATE_TOL, (where, i, rot, trans)
    rot, trans = pose_diff(oracle, po, pg)
    assert rot < SE3_TOL and trans < SE3_TOL, (where, rot, trans)


def batch_extract(c, scans, lidar, fe, f32=False):
    """loamx_extract_features_batch_dev[_f32] over a stack of scans -> per scan (edge idx, planar idx, edge xyz, planar xyz)"""
    ns, N = len(scans), scans.shape[1]
    ecap, pcap = c.edge_capacity(lidar, fe), c.planar_capacity(lidar, fe)
    d_xyz = c.alloc(scans.nbytes).upload(scans)
    d_ei, d_pi, d_ne, d_np = c.alloc(ns * ecap * 4), c.alloc(ns * pcap * 4), c.alloc(ns * 4), c.alloc(ns * 4)
    d_ex, d_px = c.alloc(ns * ecap * 24), c.alloc(ns * pcap * 24)
    try:
        c.extract_features_batch_dev(d_xyz.ptr, ns, lidar, fe, d_ei.ptr, d_ne.ptr, d_ex.ptr, d_pi.ptr, d_np.ptr, d_px.ptr, f32=f32)
        c.synchronize()
        ne, npl = d_ne.download(np.uint32, ns), d_np.download(np.uint32, ns)
        ei = d_ei.download(np.uint32, ns * ecap).reshape(ns, ecap)
        pi = d_pi.download(np.uint32, ns * pcap).reshape(ns, pcap)
        ex = d_ex.download(np.float64, ns * ecap * 3).reshape(ns, ecap, 3)
        px = d_px.download(np.float64, ns * pcap * 3).reshape(ns, pcap, 3)
    finally:
        for b in (d_xyz, d_ei, d_pi, d_ne, d_np, d_ex, d_px):
            b.free()
    assert N == lidar.scan_lines * lidar.points_per_line
    return [(ei[s, :ne[s]], pi[s, :npl[s]], ex[s, :ne[s]], px[s, :npl[s]]) for s in range(ns)]


@pytest.mark.parametrize("opt", [None] + EXTRACTION_OPTIONS)
@pytest.mark.parametrize("H,W", [(64, 1024), (128, 2048)])
def test_extraction_of_outdoor_scans(oracle, H, W, opt):
    """every scene, target and source scan: extract_features, the batch-dev entry point and the FP32 entry point (against
    the oracle on the widened scan), under every forced or optional path of the extraction"""
    c = ctx()
    lidar, fe = capi.LidarParams(H, W, 1.0, 120.0), capi.FeatureExtractionParams()
    keys = [(name, 7) for name in S.SCENES]
    scans = np.stack([s for k in keys for s in oracle_run(oracle, k, H, W)[:2]])
    want = [f for k in keys for f in (oracle_run(oracle, k, H, W)[2][:2], oracle_run(oracle, k, H, W)[2][2:])]
    wide = np.stack([s for k in keys for s in oracle_run(oracle, k, H, W, f32=True)[:2]])
    want32 = [f for k in keys for f in (oracle_run(oracle, k, H, W, True)[2][:2], oracle_run(oracle, k, H, W, True)[2][2:])]
    s32 = np.ascontiguousarray(scans.astype(np.float32))
    assert np.array_equal(s32.astype(np.float64), wide)
    with option(opt) if opt else contextlib.nullcontext():
        for s in range(len(scans)):
            e, p = c.extract_features(scans[s], lidar, fe)
            assert np.array_equal(e, want[s][0]) and np.array_equal(p, want[s][1]), (s, opt)
            e, p = c.extract_features(s32[s], lidar, fe)
            assert np.array_equal(e, want32[s][0]) and np.array_equal(p, want32[s][1]), (s, opt, "f32")
        for f32, stack, w, src in ((False, scans, want, scans), (True, s32, want32, wide)):
            for s, (ei, pi, ex, px) in enumerate(batch_extract(c, np.ascontiguousarray(stack), lidar, fe, f32)):
                assert np.array_equal(ei, w[s][0]) and np.array_equal(pi, w[s][1]), (s, opt, f32)
                assert np.array_equal(ex, src[s][w[s][0]]) and np.array_equal(px, src[s][w[s][1]]), (s, opt, f32)


# share of the lot's plane queries that round 1 queues, at the identity: 0.502 measured on the MI355X (see the docstring)
LOT_QUEUED_FLOOR = 0.25


@pytest.mark.parametrize("name", S.SCENES)
def test_association_lists_and_fits_outdoors(oracle, name):
    """loamx_associate on a 64 x 1024 pair of each scene, at the identity and at the oracle's estimate after one ICF
    iteration, under both forms of the queue chain and with / without the cooperative leftover kernel: every neighbour
    list in order, every line and plane, against the oracle (check_kind). The dump's queue counts show that the queue ran.
    Plane queries queued by round 1, measured on the MI355X: lot 50.2 % at the identity (47.6 % at the first estimate),
    canyon 18.4 %, field 28.7 % (the room: 0.5-7 %); the lot's floor is half of its measured share."""
    tgt, src, (ea, pa, eb, pb), (_, _, _, info) = oracle_run(oracle, (name, 11), 64, 1024)
    oreg = oracle.RegParams()
    est1 = oracle.pose_compose(np.array(list(info[0].update)), IDENT)
    shares = {}
    for pi, pose in enumerate((IDENT, est1)):
        for stage in ("QUEUE_ONE_STAGE", "QUEUE_TWO_STAGE"):
            for coop in (True, False):
                with option(stage), option("NO_COOP_LEFT", 0 if coop else 1):
                    dump = ctx().associate(src[eb], src[pb], tgt[ea], tgt[pa], pose)
                where = f"outdoor-{name} pose{pi} {stage} coop={coop}"
                check_kind(oracle, "edge " + where, dump, src[eb], tgt[ea], pose, False, oreg)
                n = check_kind(oracle, "plane " + where, dump, src[pb], tgt[pa], pose, True, oreg)
                assert n > 1000, where
                queued, listed = dump["plane"]["queued"]
                assert queued > 0, where  # (the queue chain had work)
                shares[(pi, stage, coop)] = queued / len(pb)
    print(name, {k: round(v, 4) for k, v in shares.items()})
    if name == "lot":
        assert shares[(0, "QUEUE_TWO_STAGE", True)] >= LOT_QUEUED_FLOOR, shares


def test_scan_pair_batch_of_outdoor_and_room_pairs(oracle):
    """16 outdoor pairs of the three scenes and 4 room pairs in ONE loamx_register_scan_pairs_dev call: per-pair grids of
    very different cell edges and per-pair queues of very different lengths share the launches. Every pair against the
    oracle; the batch's records == each pair alone == the batch in reverse order == loamx_register_scan_pairs (host in,
    host out), bit for bit; the FP32 form against the oracle on the widened scans; loamx_register_features with detail on
    the outdoor pairs (every ICF update)."""
    H, W = 64, 1024
    N = H * W
    c = ctx()
    lidar, fe, reg = capi.LidarParams(H, W, 1.0, 120.0), capi.FeatureExtractionParams(), capi.RegistrationParams()
    keys = BATCH[:6] + [("room", 31), ("room", 32)] + BATCH[6:12] + [("room", 33), ("room", 34)] + BATCH[12:]
    P = len(keys)
    host = np.ascontiguousarray(np.stack([s for k in keys for s in oracle_run(oracle, k, H, W)[:2]]))  # target first
    d_xyz, d_res = c.alloc(host.nbytes).upload(host), c.alloc(P * 64)
    c.register_scan_pairs_dev(d_xyz.ptr, P, lidar, fe, reg, d_res.ptr)
    c.synchronize()
    res = d_res.download(capi.RESULT_DTYPE, P).copy()
    for i, k in enumerate(keys):
        check_record(oracle, res[i], oracle_run(oracle, k, H, W)[3], k)
    # each pair alone
    one = c.alloc(64)
    for i in range(P):
        c.register_scan_pairs_dev(d_xyz.ptr + i * 2 * N * 24, 1, lidar, fe, reg, one.ptr)
        c.synchronize()
        assert np.array_equal(one.download(np.uint8, 64), res[i:i + 1].view(np.uint8)), keys[i]
    one.free()
    # the batch in reverse order
    rev = np.ascontiguousarray(host.reshape(P, 2, N, 3)[::-1])
    d_rev = c.alloc(rev.nbytes).upload(rev)
    c.register_scan_pairs_dev(d_rev.ptr, P, lidar, fe, reg, d_res.ptr)
    c.synchronize()
    assert np.array_equal(np.ascontiguousarray(d_res.download(capi.RESULT_DTYPE, P)[::-1]).view(np.uint8), res.view(np.uint8))
    d_rev.free()
    # host memory in, host memory out
    got = c.register_scan_pairs(host, P, lidar, fe, reg)
    assert np.array_equal(got.view(np.uint8), res.view(np.uint8))
    # float scans
    s32 = np.ascontiguousarray(host.astype(np.float32))
    d32 = c.alloc(s32.nbytes).upload(s32)
    c.register_scan_pairs_dev(d32.ptr, P, lidar, fe, reg, d_res.ptr, f32=True)
    c.synchronize()
    res32 = d_res.download(capi.RESULT_DTYPE, P).copy()
    for i, k in enumerate(keys):
        check_record(oracle, res32[i], oracle_run(oracle, k, H, W, f32=True)[3], (k, "f32"))
    assert np.array_equal(c.register_scan_pairs(s32, P, lidar, fe, reg).view(np.uint8), res32.view(np.uint8))
    for b in (d_xyz, d_res, d32):
        b.free()
    for k in BATCH:
        tgt, src, feats, oreg = oracle_run(oracle, k, H, W)
        check_detail(oracle, feats, tgt, src, oreg, k)


def test_128x2048_outdoor_pairs_through_the_scan_pair_entry_point(oracle):
    """128 x 2048 lot and canyon pairs: their planar sets exceed the 20 480-point small build, so the target sets take
    the multi-workgroup index build with 0.9-1.6 m cells"""
    H, W = 128, 2048
    c = ctx()
    lidar, fe, reg = capi.LidarParams(H, W, 1.0, 120.0), capi.FeatureExtractionParams(), capi.RegistrationParams()
    keys = [("lot", 21), ("canyon", 21)]
    host = np.ascontiguousarray(np.stack([s for k in keys for s in oracle_run(oracle, k, H, W)[:2]]))
    d_xyz, d_res = c.alloc(host.nbytes).upload(host), c.alloc(len(keys) * 64)
    c.register_scan_pairs_dev(d_xyz.ptr, len(keys), lidar, fe, reg, d_res.ptr)
    c.synchronize()
    res = d_res.download(capi.RESULT_DTYPE, len(keys))
    for i, k in enumerate(keys):
        tgt, src, feats, oreg = oracle_run(oracle, k, H, W)
        assert len(feats[1]) > 20480 and len(feats[3]) > 20480
        check_record(oracle, res[i], oreg, k)
        check_detail(oracle, feats, tgt, src, oreg, k)
    d_xyz.free()
    d_res.free()


def test_scan_to_map_along_the_canyon(oracle):
    """A map of 6 canyon scans taken 8 m apart along the street, in the world frame by their true poses, inserted one at
    a time into a target index: the outer scans first (their points leave the grid: rebuilds), then the inner ones
    (merges, until the planar kind has doubled since its last build). A seventh scan registered against the grown index
    equals the oracle on the concatenated map; the grown index equals a fresh one bit for bit; knn_search equals the
    oracle's KD-tree."""
    H, W = 64, 1024
    c = ctx()
    boxes = S.scene_boxes("canyon", 0)
    order = [0, 5, 1, 4, 2, 3]
    scans = {}
    for i in order:
        o, yaw = np.array([-20.0 + 8.0 * i, 0.3 * (i % 2), S.SENSOR_HEIGHT]), 0.01 * (i - 2)
        s = S.cast(boxes, o, yaw, H, W, S.FANS["canyon"], 0.01, np.random.default_rng([41, i]))
        e, p = oracle.extract_features(s, H, W, 1.0, 120.0)
        scans[i] = (S.to_world(s[e], o, yaw), S.to_world(s[p], o, yaw))
    map_e = np.concatenate([scans[i][0] for i in order])
    map_p = np.concatenate([scans[i][1] for i in order])
    grown = c.target_index(*scans[order[0]])
    for i in order[1:]:
        c.target_index_insert(grown, *scans[i])
    builds, merges = c.target_index_stats(grown)
    print("canyon map:", len(map_p), "planar points; full builds", builds, "merges", merges)
    assert merges >= 1 and builds >= 2 + 2, (builds, merges)  # (create builds both kinds; the planar kind is rebuilt too)
    assert c.target_index_size(grown) == (len(map_e), len(map_p))
    fresh = c.target_index(map_e, map_p)
    # the seventh scan, between the others, registered from a perturbed initial pose
    o7, yaw7 = np.array([2.5, -0.4, S.SENSOR_HEIGHT]), 0.02
    s7 = S.cast(boxes, o7, yaw7, H, W, S.FANS["canyon"], 0.01, np.random.default_rng([41, 7]))
    e7, p7 = oracle.extract_features(s7, H, W, 1.0, 120.0)
    ge, gp = c.extract_features(s7, capi.LidarParams(H, W, 1.0, 120.0))
    assert np.array_equal(ge, e7) and np.array_equal(gp, p7)
    init = S.yaw_pose(yaw7 + np.radians(1.0), o7 + np.array([0.6, 0.2, 0.0]))
    po, to, io = oracle.register_features(s7[e7], s7[p7], map_e, map_p, init)
    a = c.register_features_indexed(grown, s7[e7], s7[p7], init)
    b = c.register_features_indexed(fresh, s7[e7], s7[p7], init)
    assert a[1:] == b[1:] and np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))
    assert a[1:] == (to, io)
    rot, trans = pose_diff(oracle, po, a[0])
    assert rot < SE3_TOL and trans < SE3_TOL, (rot, trans)
    # k-NN lists of the grown index against the oracle's tree (and the fresh index)
    rng = np.random.default_rng(9)
    q = np.concatenate([S.to_world(s7[p7[rng.choice(len(p7), 280, replace=False)]], o7, yaw7), rng.uniform(-130, 130, (20, 3))])
    tree = oracle.KDTree(map_p)
    for k, radius in ((5, 2.0), (8, -1.0), (16, 2.0)):
        got, ref = c.knn_search(grown, 1, q, k, radius), c.knn_search(fresh, 1, q, k, radius)
        for i in range(len(q)):
            want = tree.knn(q[i], k, radius).astype(np.uint32)
            assert np.array_equal(got[i], want) and np.array_equal(ref[i], want), (k, radius, i)
    c.target_index_destroy(grown)
    c.target_index_destroy(fresh)


def test_host_scan_pairs_refuse_bad_arguments_before_copying():
    """Context.register_scan_pairs: ValueError (not an assert that python -O drops) for a non-contiguous or non-float
    array, too few values for n_pairs x 2 scans, and an `out` of the wrong dtype or length; nothing runs."""
    H, W, P = 16, 256, 3
    c = ctx()
    lidar = capi.LidarParams(H, W, 1.0, 120.0)
    host = np.ascontiguousarray(np.stack([capi.synth_scan_host(5, p, w, H, W, 0.01) for p in range(P) for w in (0, 1)]))
    good = c.register_scan_pairs(host, P, lidar)
    sentinel = np.zeros(P, dtype=capi.RESULT_DTYPE)
    sentinel["iterations"] = 77
    bad_calls = [
        dict(xyz=host.reshape(P * 2, H * W, 3)[:, ::2]),                   # not C-contiguous
        dict(xyz=np.asfortranarray(host.reshape(-1, 3))),                   # Fortran order
        dict(xyz=host.astype(np.float16)),                                  # neither float64 nor float32
        dict(xyz=host.reshape(-1)[:-1]),                                    # one value short
        dict(xyz=host[:2 * P - 1]),                                         # one scan short
        dict(xyz=(host.ctypes.data, np.float64)),                           # address without an element count
        dict(xyz=(host.ctypes.data, np.float64, host.size - 3)),            # an element count too small
        dict(xyz=(host.ctypes.data, np.int32, host.size)),                  # address form, wrong dtype
        dict(xyz=host, out=np.zeros(P, dtype=np.float64)),                  # out of the wrong dtype
        dict(xyz=host, out=sentinel[:P - 1]),                               # out too short
    ]
    for kw in bad_calls:
        with pytest.raises(ValueError):
            c.register_scan_pairs(kw["xyz"], P, lidar, out=kw.get("out"))
    assert (sentinel["iterations"] == 77).all()
    # the well-formed forms still run and agree
    assert np.array_equal(c.register_scan_pairs((host.ctypes.data, np.float64, host.size), P, lidar).view(np.uint8), good.view(np.uint8))
    out = np.zeros(P + 1, dtype=capi.RESULT_DTYPE)
    c.register_scan_pairs(host, P, lidar, out=out)
    assert np.array_equal(out[:P].view(np.uint8), good.view(np.uint8))
