"""GPU: the LM solve kernels (sweep_kernel, moment_kernel, lm_step_kernel, lm_pair_loop_kernel) at every form of
their record walks. Inside them the work takes different code depending on sizes and data — the first 320 edge records from LDS
and the rest from global memory; the listed plane records as a flat list in LDS, or tile by tile because they are more than 192,
or tile by tile because the call's capacity makes more than 64 tiles; evaluations from the moments or streamed; slot counts on
both sides of every chunk size — and a pose within 1e-5 of the oracle does not say which code ran. Here every scene of
tests/solve_scenes.py is ASSERTED to have its form from the library's readout (loamx_ctx_last_solve_census: listed records per
ICF iteration and per moment tile, the walk, the moments' maxima), the readout must equal the census of the CPU restatement
(tests/test_solve_forms_hostcheck.py), and the results are held to the oracle at the suite's bars (every update 1e-7, pose 1e-5)
and to each other byte for byte across entry points, capacities, batches, poisoned workspace and repeated runs."""
import numpy as np
import pytest

import hostcheck_lib as Hc
import solve_scenes as S
from gpu_common import ctx, option, pose_diff
from loam_amd import capi
from solve_forms_common import IDENT, check_expectations, cpu_census

pytestmark = pytest.mark.gpu

WALKS = {capi.WALK_FLAT: "flat", capi.WALK_TILED_BY_COUNT: "count", capi.WALK_TILED_BY_TILES: "tiles", capi.WALK_NONE: "none"}
_single = {}


def reg_of(sc, max_iterations=None):
    reg = capi.RegistrationParams()
    reg.min_associations = sc.min_assoc
    if max_iterations is not None:
        reg.max_iterations = max_iterations
    return reg


def record(pose, term, iters):
    r = np.zeros(1, capi.RESULT_DTYPE)
    r["pose"], r["termination"], r["iterations"] = pose, term, iters
    return r.view(np.uint8).copy()


def single(name):
    """the scene through the single-pair host entry point with its detail, and the census after it — once per scene"""
    if name not in _single:
        sc = S.scene(name)
        pose, term, iters, det = ctx().register_features(sc.se, sc.sp, sc.te, sc.tp, reg=reg_of(sc), want_detail=True)
        _single[name] = (pose, term, iters, det, ctx().last_solve_census(0))
    return _single[name]


def batch_dev(c, scenes, es, ps, reg, keep_census=True):
    """the scenes as ONE call of loamx_register_features_batch_dev at capacities es / ps: (result bytes [pair][64], censuses).
    (The census reads the pairs' counts from the caller's arrays: taken before they are freed.)"""
    P = len(scenes)
    bufs = []
    for k, stride in ((0, es), (1, ps), (2, es), (3, ps)):
        pts, cnt = np.zeros((P, stride, 3)), np.zeros(P, np.uint32)
        for p, sc in enumerate(scenes):
            a = (sc.se, sc.sp, sc.te, sc.tp)[k]
            pts[p, :len(a)], cnt[p] = a, len(a)
        bufs.append((c.alloc(pts.nbytes).upload(pts.view(np.uint8).reshape(-1)), c.alloc(cnt.nbytes).upload(cnt.view(np.uint8))))
    d_res = c.alloc(P * 64)
    try:
        c.register_features_batch_dev(P, bufs[0][0].ptr, bufs[0][1].ptr, bufs[1][0].ptr, bufs[1][1].ptr, bufs[2][0].ptr, bufs[2][1].ptr,
                                      bufs[3][0].ptr, bufs[3][1].ptr, es, ps, None, reg, d_res.ptr)
        c.synchronize()
        res = d_res.download(np.uint8, P * 64).reshape(P, 64).copy()
        cens = [c.last_solve_census(p) for p in range(P)] if keep_census else None
    finally:
        for b in bufs:
            b[0].free(), b[1].free()
        d_res.free()
    return res, cens


def own_strides(sc):
    return max(len(sc.se), len(sc.te), 1), max(len(sc.sp), len(sc.tp), 1)


def test_readout_errors_and_constants():
    c = capi.Context(0)
    try:
        with pytest.raises(capi.LoamxError) as e:
            c.last_solve_census(0)  # before any solve
        assert e.value.status == capi.ERR_BAD_PARAM
        sc = S.scene("flat_one")
        c.register_features(sc.se, sc.sp, sc.te, sc.tp, reg=reg_of(sc))
        cen = c.last_solve_census(0)
        assert (cen.sweep_chunk, cen.edge_cache, cen.list_cache, cen.flat_cache) == (S.SWEEP_CHUNK, S.EDGE_CACHE, S.LIST_CACHE, S.FLAT_CACHE)
        with pytest.raises(capi.LoamxError) as e:
            c.last_solve_census(1)  # one pair: out of range
        assert e.value.status == capi.ERR_BAD_PARAM
        assert c.lib.loamx_ctx_last_solve_census(c.h, 0, None) == capi.ERR_BAD_PARAM
        c.associate(sc.se, sc.sp, sc.te, sc.tp)  # (sizes the workspace anew: nothing to read any more)
        with pytest.raises(capi.LoamxError) as e:
            c.last_solve_census(0)
        assert e.value.status == capi.ERR_BAD_PARAM
    finally:
        c.close()


@pytest.mark.parametrize("name", S.NAMES)
def test_readout_equals_the_cpu_census_and_results_the_oracle(oracle, name):
    """The form of every ICF iteration from the readout (iteration i: a run with max_iterations = i + 1) equals the CPU census —
    listed records, per tile, the walk, where the moments were taken — and is the form the scene is named for; the registration
    itself against the oracle: termination, iterations, association counts of every iteration, every update within 1e-7, pose
    within 1e-5."""
    c = ctx()
    sc, stride, (_, cterm, citers, cinfo, ccen) = cpu_census(name)
    oreg = oracle.RegParams()
    oreg.min_associations = sc.min_assoc
    po, to, io, oinfo = oracle.register_features(sc.se, sc.sp, sc.te, sc.tp, None, oreg, want_info=True)
    pose, term, iters, det, cen_end = single(name)
    assert (term, iters) == (to, io) == (cterm, citers)
    assert len(det["iterations"]) == io
    worst = 0.0
    for i in range(io):
        assert (det["iterations"][i]["n_edge"], det["iterations"][i]["n_plane"]) == (oinfo[i].n_edge_assoc, oinfo[i].n_plane_assoc), (name, i)
        rot, trans = pose_diff(oracle, np.array(list(oinfo[i].update)), det["iterations"][i]["estimate_update"])
        worst = max(worst, rot, trans)
        assert rot < 1e-7 and trans < 1e-7, (name, i, rot, trans)
    rot, trans = pose_diff(oracle, po, pose)
    print("%s: worst update difference %.2e, pose difference %.2e rad / %.2e m" % (name, worst, rot, trans))
    assert rot < 1e-5 and trans < 1e-5, (name, rot, trans)
    # ---- the readout
    assert (cen_end.iterations, cen_end.termination) == (iters, term)
    assert (cen_end.n_se, cen_end.n_sp) == (len(sc.se), len(sc.sp))
    assert (cen_end.edge_stride, cen_end.planar_stride) == own_strides(sc) and stride == cen_end.planar_stride
    assert (cen_end.sweep_chunk, cen_end.edge_cache, cen_end.list_cache, cen_end.flat_cache) == (S.SWEEP_CHUNK, S.EDGE_CACHE, S.LIST_CACHE, S.FLAT_CACHE)
    live = S.live_tiles(stride, len(sc.sp))
    assert (cen_end.tiles, cen_end.live_tiles) == (S.n_tiles(stride), live)
    listed, tiles, lhs_i, lhs_u = [], [], [], []
    for i in range(iters):
        if i + 1 < iters:
            p_i, t_i, n_i = c.register_features(sc.se, sc.sp, sc.te, sc.tp, reg=reg_of(sc, i + 1))
            cen = c.last_solve_census(0)
            assert n_i == i + 1 and t_i == capi.MAX_ITER
        else:
            cen = cen_end
        assert cen.iterations == i + 1  # the workspace holds iteration i
        assert cen.use_moments == 1 and cen.mom_ref_on == (1 if i == 0 else 0), (name, i)
        assert cen.listed_total == ccen[i]["listed"], (name, i, cen.listed_total, ccen[i]["listed"])
        assert np.array_equal(cen.tile_counts, ccen[i]["tile_counts"][:live]), (name, i, cen.tile_counts, ccen[i]["tile_counts"][:live])
        assert WALKS[cen.walk] == S.walk_of(stride, ccen[i]["listed"]), (name, i)
        # (the maxima are taken over the same records with the same header arithmetic: rounding of the records' own fields only)
        assert abs(cen.s0max - ccen[i]["s0max"]) < 1e-9 and abs(cen.v2max - ccen[i]["v2max"]) < 1e-9 * max(1.0, cen.v2max), (name, i)
        ref = cen.mom_ref if cen.mom_ref_on else None
        if i == 0:
            assert np.abs(cen.mom_ref - ccen[0]["mom_ref"]).max() < 1e-9
        listed.append(cen.listed_total), tiles.append(cen.tile_counts)
        lhs_i.append(Hc.moments_bound(cen.s0max, cen.v2max, IDENT, ref)[1])
        lhs_u.append(Hc.moments_bound(cen.s0max, cen.v2max, det["iterations"][i]["estimate_update"], ref)[1])
    check_expectations(sc, stride, listed, tiles, lhs_i, lhs_u, iters)


@pytest.mark.parametrize("name", S.NAMES)
def test_capacities_options_poison_and_repeats_give_the_same_result(oracle, name):
    """The single-pair result byte for byte: through loamx_register_features_batch_dev at the pair's own capacity, at 20 481 slots
    (the scratch-based index builds) and at 65 537 (more than 64 moment tiles: the listed records tile by tile, whatever their
    number), with poisoned workspace (the tile counts nobody writes stay out of every sum), and again. NO_MOMENTS and
    NO_REF_MOMENTS (other summation orders): terminations and iteration counts equal, poses within 1e-9."""
    c = ctx()
    sc = S.scene(name)
    pose, term, iters, det, cen0 = single(name)
    want = record(pose, term, iters)
    es, ps = own_strides(sc)
    for stride in (ps, 20481, S.BIG_STRIDE):
        res, cens = batch_dev(c, [sc], es, stride, reg_of(sc))
        assert np.array_equal(res[0], want), (name, stride, res[0].view(capi.RESULT_DTYPE), want.view(capi.RESULT_DTYPE))
        cen = cens[0]
        assert (cen.planar_stride, cen.tiles, cen.n_se, cen.n_sp) == (stride, S.n_tiles(stride), len(sc.se), len(sc.sp))
        assert (cen.iterations, cen.listed_total) == (cen0.iterations, cen0.listed_total)
        assert np.array_equal(cen.tile_counts, cen0.tile_counts)
        assert WALKS[cen.walk] == S.walk_of(stride, cen0.listed_total) and (stride != S.BIG_STRIDE or cen.walk == capi.WALK_TILED_BY_TILES)
    with option("DEBUG_POISON"):
        p1, t1, i1 = c.register_features(sc.se, sc.sp, sc.te, sc.tp, reg=reg_of(sc))
        assert np.array_equal(record(p1, t1, i1), want), name
        res, _ = batch_dev(c, [sc], es, S.BIG_STRIDE, reg_of(sc), keep_census=False)
        assert np.array_equal(res[0], want), name
    for opt in ("NO_MOMENTS", "NO_REF_MOMENTS"):
        with option(opt):
            p2, t2, i2 = c.register_features(sc.se, sc.sp, sc.te, sc.tp, reg=reg_of(sc))
            cen = c.last_solve_census(0)
            c.register_features(sc.se, sc.sp, sc.te, sc.tp, reg=reg_of(sc, 1))
            first = c.last_solve_census(0)
        assert (t2, i2) == (term, iters), (name, opt)
        rot, trans = pose_diff(oracle, pose, p2)
        assert rot < 1e-9 and trans < 1e-9, (name, opt, rot, trans)
        assert first.iterations == 1 and first.mom_ref_on == 0 and first.walk == capi.WALK_NONE, (name, opt)
        if opt == "NO_MOMENTS":
            assert cen.use_moments == 0 and first.use_moments == 0 and cen.walk == capi.WALK_NONE
        else:  # five sweeps in the first iteration, the moment pass from the second on
            assert cen.use_moments == 1 and (cen.walk == capi.WALK_NONE) == (iters < 2)
            if iters >= 2:
                assert cen.listed_total == cen0.listed_total and np.array_equal(cen.tile_counts, cen0.tile_counts)
    p3, t3, i3 = c.register_features(sc.se, sc.sp, sc.te, sc.tp, reg=reg_of(sc))
    assert np.array_equal(record(p3, t3, i3), want), name
    again = c.last_solve_census(0)
    assert again.listed_total == cen0.listed_total and np.array_equal(again.tile_counts, cen0.tile_counts)


def test_one_ragged_batch_holds_every_form():
    """One pair of every form, a pair that ends with too few associations and one that converges in its first iteration, in ONE
    call: every pair's record is byte for byte what the single-pair entry point returns for it, and every pair's census is its
    own."""
    c = ctx()
    names = ["flat_none", "too_few", "flat_one", "flat_140", "count_spread", "at_once", "count_cluster", "se_321", "sp_1", "sp_4097", "changeover",
             "edge_only", "plane_only", "far_stream"]
    scenes = [S.scene(n) for n in names]
    reg = capi.RegistrationParams()
    reg.min_associations = 55  # (one value per call: too_few has 50 source points in all, sp_1 its 60 edge points)
    es, ps = max(own_strides(sc)[0] for sc in scenes), max(own_strides(sc)[1] for sc in scenes)
    runs = [batch_dev(c, scenes, es, ps, reg) for _ in range(2)]
    assert np.array_equal(runs[0][0], runs[1][0])
    res, cens = runs[0]
    for p, sc in enumerate(scenes):
        pose, term, iters = c.register_features(sc.se, sc.sp, sc.te, sc.tp, reg=reg)
        mine = c.last_solve_census(0)
        assert np.array_equal(res[p], record(pose, term, iters)), (sc.name, res[p].view(capi.RESULT_DTYPE), pose, term, iters)
        cen = cens[p]
        assert (cen.n_se, cen.n_sp, cen.iterations, cen.termination) == (len(sc.se), len(sc.sp), iters, term), sc.name
        assert (cen.planar_stride, cen.tiles, cen.live_tiles) == (ps, S.n_tiles(ps), S.live_tiles(ps, len(sc.sp))), sc.name
        assert cen.listed_total == mine.listed_total and np.array_equal(cen.tile_counts, mine.tile_counts), sc.name
        assert WALKS[cen.walk] == (S.walk_of(ps, cen.listed_total) if iters else "none"), sc.name
        assert abs(cen.s0max - mine.s0max) == 0 and abs(cen.v2max - mine.v2max) == 0, sc.name
    by = dict(zip(names, cens))
    assert (by["too_few"].termination, by["too_few"].iterations) == (capi.INSUFFICIENT_ASSOCIATIONS, 0)
    assert (by["at_once"].termination, by["at_once"].iterations, by["at_once"].mom_ref_on) == (capi.CONVERGED, 1, 1)
    assert {WALKS[cn.walk] for cn in cens} == {"none", "flat", "count"}
