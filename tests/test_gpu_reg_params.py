"""GPU: the registration across the range of loamx_reg_params, decision by decision. Every field of the struct is one
comparison somewhere in a kernel: the fit-point minima and the two gates in fit_one (register_kernels.hip), min_associations in
lm_begin_kernel, the two convergence thresholds in outer_update (reg_math.h) and max_iterations behind it, the clamps in
make_reg_config (api_core.hip). Each test puts a threshold where the CPU oracle's outcome changes and asks for the oracle's
outcome: termination and iteration count identical, association sets and nearest indices exactly the oracle's, every ICF
update within 1e-7 and the pose within 1e-5 (the bars of test_gpu_register.py). tests/test_reg_params_hostcheck.py asserts on
the CPU that the same scenes and thresholds (tests/reg_param_scenes.py) are not vacuous and how far every threshold lies from the
values it separates; the last test here writes readouts/reg_params_margins.json with the GPU's own values next to them."""
import functools
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import hostcheck_lib as Hc
import reg_param_scenes as S
from gpu_common import ctx, option, pose_diff
from loam_amd import capi
from test_gpu_direct import check_kind

pytestmark = pytest.mark.gpu

IDENT = S.IDENT
UPDATE_TOL, SE3_TOL = 1e-7, 1e-5
READOUT_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "readouts")  # (kept out of git)
READOUT = {}  # (test, field) -> one entry per threshold used: what test_zz_margins_readout writes


def note(**entry):
    READOUT[(entry["test"], entry["kind"])] = entry


def greg(**over):
    return S.params(capi.RegistrationParams, **over)


def oreg(oracle, **over):
    return S.params(oracle.RegParams, **over)


def note_sequence_threshold(name, which, thr, oracle_seq, gpu_seq):
    """a convergence threshold with the oracle's and the GPU's changes on both sides of it"""
    def sides(seq):
        seq = np.asarray(seq, dtype=np.float64)
        lo, hi = seq[seq < thr], seq[seq >= thr]
        return (float(lo.max()) if len(lo) else None), (float(hi.min()) if len(hi) else None)
    (ob, oa), (gb, ga) = sides(oracle_seq), sides(gpu_seq)
    margin = min(abs(v - thr) for v in (gb, ga) if v is not None) if (gb, ga) != (None, None) else None
    note(**dict(test=name, kind={"a": "rotation_convergence_thresh", "p": "position_convergence_thresh"}[which], threshold=thr,
                        oracle_below=ob, oracle_above=oa, gpu_below=gb, gpu_above=ga, gpu_margin=margin))


def compare_run(oracle, sets, init=None, name=None, **over):
    """one registration on the GPU and in the oracle under the same parameters, held to the bars of the module's docstring;
    returns (pose, termination, iterations, detail, the oracle's tuple)"""
    want = oracle.register_features(*sets, init, oreg(oracle, **over), want_info=True)
    po, to, io, info = want
    pg, tg, ig, det = ctx().register_features(*sets, init_pose=init, reg=greg(**over), want_detail=True)
    assert (tg, ig) == (to, io), (name, over, (tg, ig), (to, io))
    rot, trans = pose_diff(oracle, po, pg)
    assert rot < SE3_TOL and trans < SE3_TOL, (name, over, rot, trans)
    assert len(det["iterations"]) == io
    for it, (a, b) in enumerate(zip(info, det["iterations"])):
        assert (a.n_edge_assoc, a.n_plane_assoc) == (b["n_edge"], b["n_plane"]), (name, over, it)
        r, t = pose_diff(oracle, np.array(list(a.update)), b["estimate_update"])
        assert r < UPDATE_TOL and t < UPDATE_TOL, (name, over, it, r, t)
    if io:  # the association sets of the first iteration, where the estimate is the initial pose bit for bit
        est = IDENT if init is None else np.asarray(init, dtype=np.float64)
        d = det["iterations"][0]
        assert np.array_equal(d["target_T_source_init"], est)
        for pairs, src, tgt, is_plane in ((d["edge_pairs"], sets[0], sets[2], False), (d["plane_pairs"], sets[1], sets[3], True)):
            valid, nearest, _, _ = oracle.associate(src, tgt, est, is_plane, oreg(oracle, **over))
            assert np.array_equal(pairs[:, 0], np.nonzero(valid)[0]) and np.array_equal(pairs[:, 1], nearest[valid]), (name, over, is_plane)
    return pg, tg, ig, det, want


def gpu_changes(oracle, det):
    return S.changes(oracle, [d["estimate_update"] for d in det["iterations"]])


# ---- A. plane gate ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plane_fits_three_ways(oracle):
    """every source plane of room() at the identity: (dump, avg from the g++ build of the kernels' header on the dump's own
    neighbour list, avg from the library's fit entry point on the same list, the oracle's avg on the oracle's list)"""
    se, sp, te, tp = S.room()
    o_avg, o_lists = S.plane_avgs(oracle)
    dump = ctx().associate(se, sp, te, tp, IDENT, greg())
    nn = dump["plane"]["nn"]
    assert all(np.array_equal(g, o.astype(np.uint32)) for g, o in zip(nn, o_lists))
    pts = np.ascontiguousarray(np.stack([tp[l.astype(np.int64)] for l in nn]))  # (n, 5, 3)
    h = [Hc.fit_plane(p) for p in pts]
    h_prim = np.array([[*n, d] for n, d, _ in h])
    h_avg = np.array([a for _, _, a in h])
    _, _, e_avg = ctx().fit_planes(pts)
    # the association path's plane is the header's, bit for bit
    assert np.array_equal(dump["plane"]["prim"].view(np.uint64), h_prim.view(np.uint64))
    for a in (h_avg, e_avg, o_avg):
        a.setflags(write=False)
    return dump, h_avg, e_avg, o_avg


def test_plane_avg_three_ways(oracle):
    dump, h_avg, e_avg, o_avg = plane_fits_three_ways(oracle)
    assert dump["plane"]["valid"].all() and len(h_avg) > 2000
    # the fit entry point and the association path run the same arithmetic: the entry point's avg is the header's, bitwise
    assert np.array_equal(e_avg.view(np.uint64), h_avg.view(np.uint64))
    # ... and the oracle's differs from it by far less than the gaps the thresholds sit in
    assert np.abs(h_avg - o_avg).max() < S.MIN_GAP / 100, np.abs(h_avg - o_avg).max()
    assert (h_avg < 0).all()


GAP_IDS = ("q10", "q50", "q90")


@pytest.mark.parametrize("which", [0, 1, 2], ids=GAP_IDS)
def test_plane_gate_at_a_gap_threshold(oracle, which):
    thr, below, above = S.gap_thresholds(oracle)[which]
    _, h_avg, _, o_avg = plane_fits_three_ways(oracle)
    se, sp, te, tp = S.room()
    dump = ctx().associate(se, sp, te, tp, IDENT, greg(max_avg_point_plane_dist=thr))
    valid, _, _, _ = oracle.associate(sp, tp, IDENT, True, oreg(oracle, max_avg_point_plane_dist=thr))
    assert np.array_equal(dump["plane"]["valid"], valid) and np.array_equal(valid, ~(o_avg > thr))
    assert 0.05 <= 1.0 - valid.mean() <= 0.95
    note(**dict(test=f"gap threshold {GAP_IDS[which]}", kind="max_avg_point_plane_dist", threshold=thr, oracle_below=below,
                        oracle_above=above, gpu_below=float(h_avg[h_avg <= thr].max()), gpu_above=float(h_avg[h_avg > thr].min()),
                        gpu_margin=float(np.abs(h_avg - thr).min())))
    # the whole registration under that gate (compare_run holds the detail's plane_pairs to the oracle's gated set)
    compare_run(oracle, S.room(), name="gap threshold", max_avg_point_plane_dist=thr)


def test_plane_gate_on_the_edge(oracle):
    """threshold = the avg of one plane, bitwise: `avg > threshold` is strict, so the plane is valid; one ulp lower it is not"""
    _, h_avg, e_avg, _ = plane_fits_three_ways(oracle)
    i = S.edge_plane(oracle)
    assert (h_avg == h_avg[i]).sum() == 1
    assert e_avg[i].tobytes() == h_avg[i].tobytes()
    se, sp, te, tp = S.room()
    for thr, want in ((float(h_avg[i]), True), (float(np.nextafter(h_avg[i], -np.inf)), False)):
        dump = ctx().associate(se, sp, te, tp, IDENT, greg(max_avg_point_plane_dist=thr))
        assert bool(dump["plane"]["valid"][i]) == want, (thr, want)
        assert np.array_equal(dump["plane"]["valid"], ~(h_avg > thr))
        note(**dict(test=f"on the edge, plane {i} {'valid' if want else 'invalid'}", kind="max_avg_point_plane_dist", threshold=thr,
                            oracle_below=None, oracle_above=None, gpu_below=float(h_avg[h_avg <= thr].max()),
                            gpu_above=float(h_avg[h_avg > thr].min()), gpu_margin=float(np.abs(h_avg - thr).min())))


@pytest.mark.parametrize("thr", [S.INF, 0.1, 0.0, S.NAN, -S.INF], ids=str)
def test_plane_gate_special_values(oracle, thr):
    se, sp, te, tp = S.room()
    dump = ctx().associate(se, sp, te, tp, IDENT, greg(max_avg_point_plane_dist=thr))
    if thr == -S.INF:
        assert not dump["plane"]["valid"].any() and dump["edge"]["valid"].sum() > 100
        compare_run(oracle, S.room(), name="plane gate -inf", max_avg_point_plane_dist=thr)  # (edges alone)
        # fewer edges than the default min_associations: INSUFFICIENT before anything moved
        for init in (None, S.INIT_POSE):
            pg, tg, ig, det, _ = compare_run(oracle, S.small_room(), init, name="plane gate -inf, small scene", max_avg_point_plane_dist=thr)
            assert (tg, ig) == (capi.INSUFFICIENT_ASSOCIATIONS, 0) and np.array_equal(pg, IDENT if init is None else S.INIT_POSE)
    else:  # avg is negative by construction, and `avg > NaN` is false: every plane passes
        assert dump["plane"]["valid"].all()
        compare_run(oracle, S.room(), name="plane gate", max_avg_point_plane_dist=thr)


# ---- B. line gate -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cond", [0.0, 10.0, 1e300, S.DBL_MAX, S.INF, S.NAN], ids=str)
def test_line_gate(oracle, cond):
    se, sp, te, tp = S.room()
    pose = S.registered_pose(oracle)
    dump = ctx().associate(se, sp, te, tp, pose, greg(min_line_condition_number=cond))
    valid, _, _, _ = oracle.associate(se, te, pose, False, oreg(oracle, min_line_condition_number=cond))
    assert np.array_equal(dump["edge"]["valid"], valid)
    assert dump["plane"]["valid"].all()
    assert int(valid.sum()) == (0 if cond == S.INF else len(se)) and len(se) >= 200  # DBL_MAX < inf, and nothing else
    _, _, _, det, _ = compare_run(oracle, S.room(), name="line gate", min_line_condition_number=cond)
    assert all((d["n_edge"] == 0) == (cond == S.INF) for d in det["iterations"])


# ---- C. neighbour counts and fit-point minima -------------------------------------------------------------------------------
K_PAIRS = [(k, 17 - k) for k in range(1, 17)] + [(3, 4), (4, 3), (5, 6), (6, 5)]


@pytest.mark.parametrize("ke,kp", K_PAIRS)
def test_every_neighbour_count(oracle, ke, kp):
    """lists, valid sets and fits for every k from 1 to 16 on both kinds (a k below the reference's minimum of fit points
    associates nothing), on both sides of the kernels' instantiation edges 5|6 and 8|9, with the two first kernels as one
    launch (both k at most 5) and as two"""
    se, sp, te, tp = S.room()
    sp = sp[::3]  # (800 planar queries: every one is compared with a KD-tree search of the oracle)
    pose = S.registered_pose(oracle)
    over = dict(num_edge_neighbors=ke, num_plane_neighbors=kp, min_line_fit_points=2, min_plane_fit_points=3)
    dump = ctx().associate(se, sp, te, tp, pose, greg(**over))
    ce, cp = ctx().last_assoc_census("edge"), ctx().last_assoc_census("plane")
    ne = check_kind(oracle, f"edge k={ke}", dump, se, te, pose, False, oreg(oracle, **over))
    npl = check_kind(oracle, f"plane k={kp}", dump, sp, tp, pose, True, oreg(oracle, **over))
    assert ne == (len(se) if ke >= 2 else 0) and npl == (len(sp) if kp >= 3 else 0)
    instantiation = lambda k: 5 if k <= 5 else 8 if k <= 8 else 16
    assert (ce.km, cp.km) == (instantiation(ke), instantiation(kp))
    assert ce.mixed_launch == cp.mixed_launch == (1 if ke <= 5 and kp <= 5 else 0)


@pytest.mark.parametrize("is_plane", [False, True], ids=["edge", "plane"])
def test_fit_point_minimum_against_k_and_a_radius(oracle, is_plane):
    """min = k: the queries with all k neighbours inside the radius pass and the others fall short; min = k + 1: nothing can
    pass; min = 10^12: the same (the clamp to 64 in make_reg_config)"""
    se, sp, te, tp = S.room()
    pose = S.registered_pose(oracle)
    short, full = S.short_and_full(oracle, is_plane)
    assert short >= 20 and full >= 20
    k, kind = S.FIT_K[is_plane], "plane" if is_plane else "edge"
    names = ("num_plane_neighbors", "max_plane_neighbor_dist", "min_plane_fit_points") if is_plane else \
            ("num_edge_neighbors", "max_edge_neighbor_dist", "min_line_fit_points")
    for fewest, want in ((k, full), (k + 1, 0), (10 ** 12, 0)):
        over = dict(zip(names, (k, S.FIT_RADIUS[is_plane], fewest)))
        dump = ctx().associate(se, sp, te, tp, pose, greg(**over))
        valid, _, _, _ = oracle.associate(sp if is_plane else se, tp if is_plane else te, pose, is_plane, oreg(oracle, **over))
        assert np.array_equal(dump[kind]["valid"], valid) and int(valid.sum()) == want, (fewest, int(valid.sum()), want)
        counts = np.array([len(x) for x in dump[kind]["nn"]])
        assert np.array_equal(dump[kind]["valid"], counts >= min(fewest, 64))
        other = "edge" if is_plane else "plane"
        assert dump[other]["valid"].sum() > 100  # the other kind's minimum is its own
        compare_run(oracle, S.room(), pose, name=f"{kind} minimum {fewest}", **over)


def test_k_zero_for_one_kind_then_the_other(oracle):
    full = ctx().register_features(*S.room(), want_detail=True)[3]["iterations"][0]
    for over, dead in ((dict(num_edge_neighbors=0, min_line_fit_points=1), "edge"), (dict(num_plane_neighbors=0, min_plane_fit_points=2), "plane")):
        pg, tg, ig, det, _ = compare_run(oracle, S.room(), name="k = 0", **over)
        assert tg == capi.CONVERGED
        live = "plane" if dead == "edge" else "edge"
        assert all(d["n_" + dead] == 0 and d["n_" + live] > 100 for d in det["iterations"])
        assert np.array_equal(det["iterations"][0][live + "_pairs"], full[live + "_pairs"])  # the other kind is unaffected
        dump = ctx().associate(*S.room(), IDENT, greg(**over))
        assert not dump[dead]["valid"].any() and all(len(x) == 0 for x in dump[dead]["nn"])
        # the same minimum with a k above 0 is refused
        refused = dict(over, **{("num_edge_neighbors" if dead == "edge" else "num_plane_neighbors"): 5})
        with pytest.raises(capi.LoamxError) as e:
            ctx().register_features(*S.room(), reg=greg(**refused))
        assert e.value.status == capi.ERR_BAD_PARAM


def test_walls(oracle):
    for over in (dict(num_edge_neighbors=17), dict(num_plane_neighbors=17), dict(max_iterations=1001)):
        for call in (lambda r: ctx().register_features(*S.small_room(), reg=r), lambda r: ctx().associate(*S.small_room(), IDENT, r),
                     lambda r: ctx().registration_information(*S.small_room(), reg=r)):
            with pytest.raises(capi.LoamxError) as e:
                call(greg(**over))
            assert e.value.status == capi.ERR_UNSUPPORTED, over
    compare_run(oracle, S.small_room(), name="after the walls", num_edge_neighbors=16, num_plane_neighbors=16, max_iterations=1000)


# ---- D. convergence thresholds ----------------------------------------------------------------------------------------------
CASE_ITERATIONS = {"rot_binds_1": 2, "rot_binds_2": 3, "pos_binds_1": 2, "pos_binds_2": 3, "rot_1_pos_3": 4, "rot_3_pos_1": 4,
                   "rot_2_pos_1": 3, "rot_1_pos_1": 2}


@pytest.mark.parametrize("name", list(CASE_ITERATIONS))
def test_convergence_thresholds(oracle, name):
    """one threshold binds (the other +inf), or both at different iterations; the iteration count is the one the oracle's change
    sequences a_0 > a_1 > ..., p_0 > p_1 > ... give for the thresholds, which lie between two of their values"""
    a, p = S.convergence_sequence(oracle)
    rot, pos = S.convergence_cases(oracle)[name]
    assert S.iterations_by_sequence(a, p, rot, pos, 10) == (CASE_ITERATIONS[name], True)
    pg, tg, ig, det, _ = compare_run(oracle, S.room(), name=name, rotation_convergence_thresh=rot, position_convergence_thresh=pos)
    assert (tg, ig) == (capi.CONVERGED, CASE_ITERATIONS[name])
    ga, gp = gpu_changes(oracle, det)
    for which, thr, oseq, gseq in (("a", rot, a, ga), ("p", pos, p, gp)):
        if np.isfinite(thr):
            note_sequence_threshold(name, which, thr, oseq[:ig], gseq)
    if name in S.SWAP_SHOWN_BY:  # the two numbers exchanged stop the run elsewhere: an exchange on the way to the kernel would show
        sg = compare_run(oracle, S.room(), name=name + " exchanged", rotation_convergence_thresh=pos, position_convergence_thresh=rot)
        assert sg[2] != ig


@pytest.mark.parametrize("scene", ["same", "moved"])
@pytest.mark.parametrize("thr", [0.0, -1.0, S.NAN], ids=str)
def test_thresholds_that_nothing_is_below_run_to_the_limit(oracle, scene, thr):
    """0 < 0 is false, and so is anything < -1 and anything < NaN: MAX_ITER after max_iterations, whatever the updates"""
    sets = S.same_room() if scene == "same" else S.room()
    for m in (1, 2, 3, 7):
        pg, tg, ig, det, _ = compare_run(oracle, sets, name="to the limit", max_iterations=m, rotation_convergence_thresh=thr,
                                         position_convergence_thresh=thr)
        assert (tg, ig) == (capi.MAX_ITER, m)
    updates = [d["estimate_update"] for d in det["iterations"]]
    first = next(i for i, u in enumerate(updates) if np.array_equal(u, IDENT))  # (the hostcheck test: the oracle reaches it)
    assert all(np.array_equal(u, IDENT) for u in updates[first:])  # once the LM returns the identity update, nothing moves


def test_infinite_thresholds_converge_after_one_iteration(oracle):
    for sets in (S.room(), S.same_room()):
        pg, tg, ig, det, _ = compare_run(oracle, sets, name="inf", rotation_convergence_thresh=S.INF, position_convergence_thresh=S.INF)
        assert (tg, ig) == (capi.CONVERGED, 1)


def test_a_thousand_iterations(oracle):
    """max_iterations at its wall on the smallest scene: 1000 detail entries (the pair * max_iterations + iteration indexing of
    the iteration records) and the oracle's pose"""
    pg, tg, ig, det, _ = compare_run(oracle, S.small_room(), name="1000 iterations", max_iterations=1000, rotation_convergence_thresh=0.0,
                                     position_convergence_thresh=0.0)
    assert (tg, ig, len(det["iterations"])) == (capi.MAX_ITER, 1000, 1000)


# ---- E. min_associations ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("init", [None, S.INIT_POSE], ids=["identity", "moved"])
def test_min_associations_boundary_at_the_first_iteration(oracle, init):
    _, _, _, info = oracle.register_features(*S.room(), init, oreg(oracle, min_associations=0), want_info=True)
    c0 = int(info[0].n_edge_assoc + info[0].n_plane_assoc)
    pg, tg, ig, det, _ = compare_run(oracle, S.room(), init, name="c0", min_associations=c0)  # ne + np < min is strict
    assert tg != capi.INSUFFICIENT_ASSOCIATIONS and det["iterations"][0]["n_edge"] + det["iterations"][0]["n_plane"] == c0
    for fewest in (c0 + 1, 2 ** 40):  # (2^40: the clamp to 2^32 - 1)
        pg, tg, ig, det, _ = compare_run(oracle, S.room(), init, name="c0 + 1", min_associations=fewest)
        assert (tg, ig) == (capi.INSUFFICIENT_ASSOCIATIONS, 0)
        assert pg.tobytes() == (IDENT if init is None else S.INIT_POSE).tobytes()


def test_min_associations_mid_run(oracle):
    """the decoy scene's count falls after the first and after the second update: the run ends INSUFFICIENT there, with the
    estimate of the updates made so far"""
    c = S.decoy_counts(oracle)
    assert c[1] < c[0] and c[2] < c[1]
    for fewest, want in ((c[0], 1), (c[1] + 1, 1), (c[1], 2)):
        pg, tg, ig, det, (po, _, _, info) = compare_run(oracle, S.decoy(), name="decoy", **{**S.DECOY_OVER, "min_associations": fewest})
        assert (tg, ig) == (capi.INSUFFICIENT_ASSOCIATIONS, want)
        est = IDENT
        for d in det["iterations"]:
            est = oracle.pose_compose(d["estimate_update"], est)
        rot, trans = pose_diff(oracle, est, pg)
        assert rot < 1e-12 and trans < 1e-12 and not np.array_equal(pg, IDENT)  # the estimate after that many updates
        assert [d["n_edge"] + d["n_plane"] for d in det["iterations"]] == c[:want]


# ---- F. one batch, every ending ---------------------------------------------------------------------------------------------
def run_batch(scenes, reg):
    c, P = ctx(), len(scenes)
    es = max(max(len(s[0]), len(s[2])) for s in scenes)
    ps = max(max(len(s[1]), len(s[3])) for s in scenes)
    bufs = []
    for k, stride in ((0, es), (1, ps), (2, es), (3, ps)):
        pts, cnt = np.zeros((P, stride, 3)), np.zeros(P, np.uint32)
        for p, s in enumerate(scenes):
            pts[p, :len(s[k])], cnt[p] = s[k], len(s[k])
        bufs.append((c.alloc(pts.nbytes).upload(pts.view(np.uint8).reshape(-1)), c.alloc(cnt.nbytes).upload(cnt.view(np.uint8))))
    d_res = c.alloc(P * 64)
    try:
        c.register_features_batch_dev(P, bufs[0][0].ptr, bufs[0][1].ptr, bufs[1][0].ptr, bufs[1][1].ptr, bufs[2][0].ptr, bufs[2][1].ptr,
                                      bufs[3][0].ptr, bufs[3][1].ptr, es, ps, None, reg, d_res.ptr)
        c.synchronize()
        return d_res.download(np.uint8, P * 64).reshape(P, 64).copy()
    finally:
        for b in bufs:
            b[0].free(), b[1].free()
        d_res.free()


def test_one_batch_with_every_ending(oracle):
    """eleven pairs under one parameter set off its defaults in seven fields: CONVERGED after 1, 2, 3 and 4 iterations, MAX_ITER,
    INSUFFICIENT before the first and before the second iteration, so that the live-pair deal of iterations 3+ sees pairs leave in
    every way. Every record is the pair's own single-pair call, byte for byte, also under NO_LIVE_DEAL, under DEBUG_POISON and for
    the batch reversed."""
    scenes = [scene() for scene, _ in S.BATCH]
    reg = greg(**S.BATCH_OVER)
    assert len(scenes) >= 9
    res = run_batch(scenes, reg)
    rec = res.view(capi.RESULT_DTYPE).reshape(-1)
    endings = [(int(r["termination"]), int(r["iterations"])) for r in rec]
    assert endings == [want for _, want in S.BATCH], endings
    for ending in S.BATCH_ENDINGS:
        assert ending in endings
    for p, s in enumerate(scenes):
        single = capi.RegResult()
        pose, term, iters = ctx().register_features(*s, reg=reg)
        single.pose[:], single.termination, single.iterations = list(pose), term, iters
        assert bytes(single) == res[p].tobytes(), p
        po, to, io = oracle.register_features(*s, None, oreg(oracle, **S.BATCH_OVER))
        rot, trans = pose_diff(oracle, po, rec[p]["pose"])
        assert (to, io) == endings[p] and rot < SE3_TOL and trans < SE3_TOL, (p, rot, trans)
    with option("NO_LIVE_DEAL"):
        assert np.array_equal(run_batch(scenes, reg), res)
    with option("DEBUG_POISON"):
        assert np.array_equal(run_batch(scenes, reg), res)
    assert np.array_equal(run_batch(scenes[::-1], reg)[::-1], res)


# ---- G. bindings ------------------------------------------------------------------------------------------------------------
def shim_register(sets, over):
    """the scene and the twelve fields through the C++ shim (include/loam/registration.h): tests/cpp/test_shim in its file mode,
    a child process. Returns (pose, termination, [(n_edge, n_plane)] per iteration)."""
    from test_gpu_cpp_shim import build_shim_test
    exe = build_shim_test()
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(src, "wb") as f:
            f.write(np.array([len(s) for s in sets], dtype=np.uint64).tobytes())
            f.write(bytes(S.params(capi.RegistrationParams, **over)))
            f.write(IDENT.tobytes())
            for s in sets:
                f.write(np.ascontiguousarray(s, dtype=np.float64).tobytes())
        out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-1000:])
        raw = np.fromfile(dst, dtype=np.uint8)
    pose = raw[:56].view(np.float64).copy()
    words = raw[56:].view(np.uint64)
    n = int(words[1])
    return pose, int(words[0]), [(int(words[2 + 2 * i]), int(words[3 + 2 * i])) for i in range(n)]


@pytest.mark.parametrize("name", ["converged", "insufficient", "max_iter"])
def test_all_twelve_fields_through_capi_and_the_cpp_shim(oracle, name):
    """Parameter sets with all twelve fields off their defaults and pairwise distinct; for every field there is a set in which
    the oracle's result changes when that field alone is reset (reg_param_scenes.binding_sets says why no one set can do that;
    the hostcheck test asserts it by oracle runs): a field dropped, defaulted or exchanged with another on the way to the kernels
    shows against the oracle. The C++ shim returns the bytes capi returns."""
    over = S.binding_sets(oracle)[name]
    pg, tg, ig, det, _ = compare_run(oracle, S.binding_room(), name=name, **over)
    assert (tg, ig) == {"converged": (capi.CONVERGED, 2), "insufficient": (capi.INSUFFICIENT_ASSOCIATIONS, 0), "max_iter": (capi.MAX_ITER, 1)}[name]
    pose, term, counts = shim_register(S.binding_room(), over)
    assert pose.tobytes() == pg.tobytes() and term == tg
    assert counts == [(d["n_edge"], d["n_plane"]) for d in det["iterations"]]


# ---- H. readout -------------------------------------------------------------------------------------------------------------
def test_zz_margins_readout(oracle):
    """runs last in this module: every threshold used with the oracle's values on both sides of it, the GPU's own values (avg from
    the dump's neighbour lists through the header's g++ build, angle and position changes from the detail's updates) and the
    smallest distance of a GPU value from a threshold. A threshold closer to the GPU's value than to the oracle's shows here.
    The tests that place a threshold note it as they run; those that have not run in this session are run from here."""
    producers = [(test_plane_gate_at_a_gap_threshold, (w,), f"gap threshold {q}") for w, q in enumerate(GAP_IDS)]
    producers += [(test_plane_gate_on_the_edge, (), f"on the edge, plane {S.edge_plane(oracle)} valid")]
    producers += [(test_convergence_thresholds, (name,), name) for name in CASE_ITERATIONS]
    for fn, args, noted_as in producers:
        if not any(test == noted_as for test, _ in READOUT):
            fn(oracle, *args)
    entries = list(READOUT.values())
    assert len(entries) == 3 + 2 + 12
    margins = [r["gpu_margin"] for r in entries if not r["test"].startswith("on the edge")]
    table = dict(thresholds=entries, smallest_gpu_margin=min(margins))
    os.makedirs(READOUT_DIR, exist_ok=True)
    with open(os.path.join(READOUT_DIR, "reg_params_margins.json"), "w") as f:
        json.dump(table, f, indent=1)
    print(json.dumps(table))
    for r in entries:
        if r["test"].startswith("on the edge"):
            continue
        # the GPU's values lie on the oracle's side of every threshold, no closer to it than half the oracle's own distance
        for side in ("below", "above"):
            o, g = r["oracle_" + side], r["gpu_" + side]
            if o is not None:
                assert g is not None and abs(g - r["threshold"]) >= 0.5 * abs(o - r["threshold"]), r
