"""CPU: the scenes and thresholds of tests/test_gpu_reg_params.py are not vacuous and have the margins that test relies on.
Everything here is asserted on the CPU oracle (no GPU): the gaps the plane-gate thresholds sit in and the share of planes
each rejects, the decreasing convergence sequences and the distance of every threshold from its neighbours, the falling
association counts of the decoy scene, the queries on both sides of the fit-point minima, the endings of the batch, and the
fields of the binding parameter sets that change the oracle's result when reset. The g++ build of the kernels' own header
(tests/hostcheck) is run over the same cases where it has the decision: the gates and the convergence test of reg_math.h."""
import math

import numpy as np
import pytest

import hostcheck_lib as Hc
import reg_param_scenes as S

IDENT = S.IDENT


def run(oracle, sets, init=None, **over):
    return oracle.register_features(*sets, init, S.params(oracle.RegParams, **over), want_info=True)


# ---- A. plane gate ----------------------------------------------------------------------------------------------------------
def test_avg_dist_is_never_positive_on_the_noisy_scene(oracle):
    """fitPlane's residual is orthogonal to the columns of P, so its sum is -|r|^2: the default gate 0.1, and 0.0, reject nothing"""
    avg, lists = S.plane_avgs(oracle)
    assert len(avg) > 2000 and not np.isnan(avg).any() and all(len(l) == 5 for l in lists)
    assert (avg < 0).all() and avg.max() > -1e-8 and avg.min() < -1e-3  # (seven decades of spread)
    sp, tp = S.room()[1], S.room()[3]
    for thr in (S.INF, 0.1, 0.0, S.NAN):  # avg > NaN is false: everything passes
        valid, _, _, _ = oracle.associate(sp, tp, IDENT, True, S.params(oracle.RegParams, max_avg_point_plane_dist=thr))
        assert valid.all(), thr
    valid, _, _, _ = oracle.associate(sp, tp, IDENT, True, S.params(oracle.RegParams, max_avg_point_plane_dist=-S.INF))
    assert not valid.any()
    pose, term, iters, _ = run(oracle, S.room(), max_avg_point_plane_dist=-S.INF, min_associations=len(S.room()[0]) + 1)
    assert (term, iters) == (oracle.INSUFFICIENT_ASSOCIATIONS, 0) and np.array_equal(pose, IDENT)


def test_gap_thresholds_sit_in_gaps_and_reject_a_share(oracle):
    avg, _ = S.plane_avgs(oracle)
    got = S.gap_thresholds(oracle)
    assert len({t for t, _, _ in got}) == 3
    for (thr, below, above), q in zip(got, (0.1, 0.5, 0.9)):
        assert above - below >= S.MIN_GAP and thr - below >= S.MIN_GAP / 2 and above - thr >= S.MIN_GAP / 2
        assert not ((avg > below) & (avg < above)).any()  # nothing else inside the gap
        rejected = float((avg > thr).mean())
        assert 0.05 <= rejected <= 0.95 and abs(rejected - (1 - q)) < 0.02, (q, rejected)
        valid, _, _, _ = oracle.associate(S.room()[1], S.room()[3], IDENT, True, S.params(oracle.RegParams, max_avg_point_plane_dist=thr))
        assert np.array_equal(valid, ~(avg > thr))
        # the g++ build of the kernels' header takes the same decision for every plane
        hv, _, _, _ = Hc.associate(S.room()[1], S.room()[3], IDENT, True, S.params(Hc.RegParams, max_avg_point_plane_dist=thr))
        assert np.array_equal(hv, valid)


def test_the_on_the_edge_plane_has_an_avg_of_its_own(oracle):
    avg, lists = S.plane_avgs(oracle)
    i = S.edge_plane(oracle)
    assert (avg == avg[i]).sum() == 1 and 0.05 <= float((avg > avg[i]).mean()) <= 0.95
    tp = S.room()[3]
    h = np.array([Hc.fit_plane(tp[l])[2] for l in lists])
    assert (h == h[i]).sum() == 1  # ... in the header's arithmetic too
    # strictness on the CPU build: at the value itself the plane passes, one ulp below it does not
    for thr, want in ((h[i], True), (np.nextafter(h[i], -np.inf), False)):
        hv, _, _, _ = Hc.associate(S.room()[1], tp, IDENT, True, S.params(Hc.RegParams, max_avg_point_plane_dist=float(thr)))
        assert hv[i] == want and np.array_equal(hv, ~(h > thr))


# ---- B. line gate -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cond", [0.0, 10.0, 1e300, S.DBL_MAX, S.INF, S.NAN], ids=str)
def test_line_gate_rejects_only_at_infinity(oracle, cond):
    se, sp, te, tp = S.room()
    pose = S.registered_pose(oracle)
    base, _, _, _ = oracle.associate(se, te, pose, False, S.params(oracle.RegParams))
    assert base.sum() >= 200
    valid, _, _, _ = oracle.associate(se, te, pose, False, S.params(oracle.RegParams, min_line_condition_number=cond))
    hv, _, _, _ = Hc.associate(se, te, pose, False, S.params(Hc.RegParams, min_line_condition_number=cond))
    assert np.array_equal(hv, valid)
    if cond == S.INF:
        assert not valid.any()
        planes, _, _, _ = oracle.associate(sp, tp, pose, True, S.params(oracle.RegParams, min_line_condition_number=cond))
        assert planes.all()  # planes untouched
    else:
        assert np.array_equal(valid, base)


# ---- C. fit-point minima ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is_plane", [False, True], ids=["edge", "plane"])
def test_the_radius_leaves_queries_on_both_sides_of_the_minimum(oracle, is_plane):
    short, full = S.short_and_full(oracle, is_plane)
    assert short >= 20 and full >= 20, (short, full)
    se, sp, te, tp = S.room()
    src, tgt = (sp, tp) if is_plane else (se, te)
    k, names = S.FIT_K[is_plane], (("num_plane_neighbors", "max_plane_neighbor_dist", "min_plane_fit_points") if is_plane else
                                   ("num_edge_neighbors", "max_edge_neighbor_dist", "min_line_fit_points"))
    counts = {}
    for fewest in (k, k + 1, 10 ** 12):
        over = dict(zip(names, (k, S.FIT_RADIUS[is_plane], fewest)))
        valid, _, _, _ = oracle.associate(src, tgt, S.registered_pose(oracle), is_plane, S.params(oracle.RegParams, **over))
        counts[fewest] = int(valid.sum())
    assert counts == {k: full, k + 1: 0, 10 ** 12: 0}


def test_k_zero_leaves_the_other_kind_alone(oracle):
    full = run(oracle, S.room())
    for over, dead in ((dict(num_edge_neighbors=0, min_line_fit_points=1), 0), (dict(num_plane_neighbors=0, min_plane_fit_points=2), 1)):
        pose, term, iters, info = run(oracle, S.room(), **over)
        assert term == oracle.CONVERGED
        for a, b in zip(info, full[3]):
            n = (a.n_edge_assoc, a.n_plane_assoc)
            assert n[dead] == 0 and n[1 - dead] > 100
        assert (info[0].n_edge_assoc, info[0].n_plane_assoc)[1 - dead] == (full[3][0].n_edge_assoc, full[3][0].n_plane_assoc)[1 - dead]


# ---- D. convergence thresholds ----------------------------------------------------------------------------------------------
def test_convergence_sequences_decrease_and_every_threshold_has_its_margins(oracle):
    a, p = S.convergence_sequence(oracle)
    for seq in (a, p):
        nz = [x for x in seq if x > 0]
        assert len(nz) >= 5 and seq[:len(nz)] == nz and all(x == 0 for x in seq[len(nz):])  # decreasing until exactly 0, then 0
        assert all(nz[i] > nz[i + 1] for i in range(len(nz) - 1))
    cases = S.convergence_cases(oracle)
    used = S.thresholds_used(cases)
    assert len(used) == 12
    for name, which, thr in used:
        below, above, dist, ratio = S.margins(a if which == "a" else p, thr)
        assert below < thr < above
        assert dist >= 1e-5, (name, which, thr, dist)              # 100 x the 1e-7 update bar
        assert ratio >= math.sqrt(2) * (1 - 1e-12), (name, which, thr, ratio)


def test_convergence_cases_end_where_the_sequence_says(oracle):
    a, p = S.convergence_sequence(oracle)
    want = {"rot_binds_1": 2, "rot_binds_2": 3, "pos_binds_1": 2, "pos_binds_2": 3, "rot_1_pos_3": 4, "rot_3_pos_1": 4,
            "rot_2_pos_1": 3, "rot_1_pos_1": 2}
    cases = S.convergence_cases(oracle)
    assert set(cases) == set(want)
    for name, (rot, pos) in cases.items():
        assert S.iterations_by_sequence(a, p, rot, pos, 10) == (want[name], True), name
        pose, term, iters, _ = run(oracle, S.room(), rotation_convergence_thresh=rot, position_convergence_thresh=pos)
        assert (term, iters) == (oracle.CONVERGED, want[name]), name
        hp, ht, hi = Hc.register(*S.room(), prm=S.params(Hc.RegParams, rotation_convergence_thresh=rot, position_convergence_thresh=pos))
        assert (ht, hi) == (term, iters), name
    # what shows an exchange of the two thresholds: with the two numbers of a run exchanged the oracle stops elsewhere
    for name in S.SWAP_SHOWN_BY:
        rot, pos = cases[name]
        _, term, iters, _ = run(oracle, S.room(), rotation_convergence_thresh=pos, position_convergence_thresh=rot)
        assert iters != want[name], name


@pytest.mark.parametrize("scene", ["same", "moved"])
def test_thresholds_zero_run_to_the_limit(oracle, scene):
    sets = S.same_room() if scene == "same" else S.room()
    for m in (1, 2, 3, 7):
        for thr in (0.0, -1.0, S.NAN):
            pose, term, iters, info = run(oracle, sets, max_iterations=m, rotation_convergence_thresh=thr, position_convergence_thresh=thr)
            assert (term, iters) == (oracle.MAX_ITER, m), (m, thr)
        updates = S.oracle_updates(info)
        first = next((i for i, u in enumerate(updates) if np.array_equal(u, IDENT)), None)
        if first is not None:  # once the LM returns the identity, nothing moves any more
            assert all(np.array_equal(u, IDENT) for u in updates[first:])
    assert first is not None  # (seven iterations reach it on both scenes)
    pose, term, iters, _ = run(oracle, sets, rotation_convergence_thresh=S.INF, position_convergence_thresh=S.INF)
    assert (term, iters) == (oracle.CONVERGED, 1)


def test_degenerate_thresholds_in_the_header_build(oracle):
    """the convergence test of reg_math.h (outer_update) built with g++, on the values a comparison can get wrong"""
    for thr, want in ((0.0, (oracle.MAX_ITER, 3)), (-1.0, (oracle.MAX_ITER, 3)), (S.NAN, (oracle.MAX_ITER, 3)), (S.INF, (oracle.CONVERGED, 1))):
        over = dict(max_iterations=3, rotation_convergence_thresh=thr, position_convergence_thresh=thr)
        _, term, iters, _ = run(oracle, S.room(), **over)
        _, ht, hi = Hc.register(*S.room(), prm=S.params(Hc.RegParams, **over))
        assert (term, iters) == want and (ht, hi) == want, thr


def test_a_thousand_iterations_on_the_smallest_scene(oracle):
    sets = S.small_room()
    assert 50 <= len(sets[0]) <= 70 and 250 <= len(sets[1]) <= 350
    pose, term, iters, info = run(oracle, sets, max_iterations=1000, rotation_convergence_thresh=0.0, position_convergence_thresh=0.0)
    assert (term, iters, len(info)) == (oracle.MAX_ITER, 1000, 1000)
    assert info[0].n_edge_assoc + info[0].n_plane_assoc >= 100


# ---- E. min_associations ----------------------------------------------------------------------------------------------------
def test_the_decoy_scene_loses_associations_update_by_update(oracle):
    c = S.decoy_counts(oracle)
    assert len(c) == 4 and c[1] < c[0] and c[2] < c[1], c
    assert c[0] - c[1] >= 100  # the patch, not a stray query
    d = S.decoy()
    assert 2000 <= len(d[1]) <= 3000 and len(d[0]) <= 300
    for fewest, want in ((c[0], 1), (c[1] + 1, 1), (c[1], 2)):
        pose, term, iters, info = run(oracle, d, **{**S.DECOY_OVER, "min_associations": fewest})
        assert (term, iters) == (oracle.INSUFFICIENT_ASSOCIATIONS, want), (fewest, term, iters)
    pose, term, iters, _ = run(oracle, d, **{**S.DECOY_OVER, "min_associations": c[0] + 1})
    assert (term, iters) == (oracle.INSUFFICIENT_ASSOCIATIONS, 0) and np.array_equal(pose, IDENT)


def test_the_boundary_at_iteration_zero(oracle):
    for init in (None, S.INIT_POSE):
        _, _, _, info = run(oracle, S.room(), init, min_associations=0)
        c0 = info[0].n_edge_assoc + info[0].n_plane_assoc
        assert c0 > 1000
        pose, term, iters, _ = run(oracle, S.room(), init, min_associations=c0)
        assert term != oracle.INSUFFICIENT_ASSOCIATIONS and iters >= 1
        for fewest in (c0 + 1, 2 ** 40):
            pose, term, iters, _ = run(oracle, S.room(), init, min_associations=fewest)
            assert (term, iters) == (oracle.INSUFFICIENT_ASSOCIATIONS, 0)
            assert np.array_equal(pose, IDENT if init is None else S.INIT_POSE)


# ---- F. the batch -----------------------------------------------------------------------------------------------------------
def test_the_batch_holds_every_ending(oracle):
    assert len(S.BATCH) >= 9
    got = []
    for p, (scene, want) in enumerate(S.BATCH):
        pose, term, iters, info = run(oracle, scene(), **S.BATCH_OVER)
        assert (term, iters) == want, (p, term, iters)
        got.append((term, iters))
        # no change of any iteration sits within 1e-5 (100 x the update bar) of its threshold
        a, pp = S.changes(oracle, S.oracle_updates(info))
        assert all(abs(x - S.BATCH_OVER["rotation_convergence_thresh"]) >= 1e-5 for x in a), (p, a)
        assert all(abs(x - S.BATCH_OVER["position_convergence_thresh"]) >= 1e-5 for x in pp), (p, pp)
    for ending in S.BATCH_ENDINGS:
        assert ending in got, ending
    assert sum(it >= 3 for _, it in got) >= 2 and sum(it <= 2 for _, it in got) >= 2  # the live-pair deal has pairs to drop and to keep
    off_default = [f for f in S.REG_FIELDS if S.BATCH_OVER.get(f, S.DEFAULTS[f]) != S.DEFAULTS[f]]
    assert len(off_default) >= 7


# ---- G. bindings ------------------------------------------------------------------------------------------------------------
def test_binding_sets_are_off_default_distinct_and_every_field_matters_in_one(oracle):
    sets = S.binding_sets(oracle)
    assert set(sets) == set(S.BINDING_COVERS) and sorted(f for v in S.BINDING_COVERS.values() for f in v) == sorted(S.REG_FIELDS)
    for name, over in sets.items():
        assert set(over) == set(S.REG_FIELDS)
        values = [float(over[f]) for f in S.REG_FIELDS]
        assert all(over[f] != S.DEFAULTS[f] for f in S.REG_FIELDS), name
        assert len(set(values)) == 12, (name, values)
        assert over["max_avg_point_plane_dist"] < 0  # the plane gate acts
    # the sets' own thresholds have the margins of sections A and D: the plane gate in a gap of the oracle's avg values under
    # these neighbour parameters, the convergence thresholds 1e-5 and a factor sqrt(2) from every change of the oracle's run
    over = sets["converged"]
    avg, _ = S.avgs_of(oracle, S.binding_room()[1], S.binding_room()[3], over["num_plane_neighbors"], over["max_plane_neighbor_dist"],
                       over["min_plane_fit_points"])
    avg = avg[~np.isnan(avg)]
    gate = over["max_avg_point_plane_dist"]
    assert np.abs(avg - gate).min() >= S.MIN_GAP / 2 and 0.05 <= float((avg > gate).mean()) <= 0.95
    a, p = S.sequence_of(oracle, S.binding_room(), **over)
    rot, pos = over["rotation_convergence_thresh"], over["position_convergence_thresh"]
    below, above, dist, ratio = S.margins(a, rot)
    assert (below, above) == (a[1], a[0]) and dist >= 1e-5 and ratio >= math.sqrt(2)
    assert pos > max(p) and pos - max(p) >= 1e-5 and pos / max(p) >= math.sqrt(2)  # (above every position change)
    assert S.iterations_by_sequence(a, p, rot, pos, 11) == (2, True)
    base = {name: S.signature(oracle, S.binding_room(), S.params(oracle.RegParams, **over)) for name, over in sets.items()}
    assert [base[n][:2] for n in ("converged", "insufficient", "max_iter")] == [(oracle.CONVERGED, 2), (oracle.INSUFFICIENT_ASSOCIATIONS, 0),
                                                                                (oracle.MAX_ITER, 1)]
    # twelve oracle runs: each field reset to its default, in the set that covers it, changes the result
    for name, covered in S.BINDING_COVERS.items():
        for f in covered:
            reset = S.signature(oracle, S.binding_room(), S.params(oracle.RegParams, **{**sets[name], f: S.DEFAULTS[f]}))
            assert S.differs(oracle, base[name], reset), (name, f, base[name][:3], reset[:3])
    # ... and so does the exchange of the two radii, of the two convergence thresholds and of each with the double next to it
    over = sets["converged"]
    for f, g in (("max_edge_neighbor_dist", "max_plane_neighbor_dist"), ("rotation_convergence_thresh", "position_convergence_thresh"),
                 ("max_plane_neighbor_dist", "max_avg_point_plane_dist"), ("max_edge_neighbor_dist", "min_line_condition_number"),
                 ("max_avg_point_plane_dist", "rotation_convergence_thresh")):
        swapped = S.signature(oracle, S.binding_room(), S.params(oracle.RegParams, **{**over, f: over[g], g: over[f]}))
        assert S.differs(oracle, base["converged"], swapped), (f, g)
