"""CPU: every scene of tests/assoc_scenes.py takes the route it was built for, by the g++ build of the kernels' own functions
(tests/hostcheck: hostcheck_knn_routes walks a query through round 1, the rest kernel's searches and the keyed search in the
kernels' order). tests/test_gpu_assoc_routes.py asserts that the census of loamx_associate EQUALS these numbers; here a scene
that has gone vacuous — a predicate moved, a constant changed — fails on a machine without a GPU. Last: the census checks
(assoc_scenes.check_census) refuse a wrong census."""
import copy

import numpy as np
import pytest

import assoc_scenes as S


def counts(s, one_stage=False, coop=True, handoff=False):
    q, t, k, r = S.sets(s)
    R = S.routes(s, handoff)
    return R, S.expected(R, len(t), one_stage, coop)


def test_wall_is_finished_by_round_one():
    s = S.wall()
    R, e = counts(s, handoff=True)
    assert e["queued"] == 0 and e["unverified"] == len(s.src_p) == 667 and e["late"] <= 3  # (the mixed launch: every count word a selection)
    assert abs(R["h"] - np.sqrt(8 * 2 * 24 / 2000)) < 0.01 and R["dims"][1] == 1


@pytest.mark.parametrize("k", [3, 5, 6, 8, 9, 16])
def test_sparse_is_queued_on_the_guard_and_split_by_the_lean_search(k):
    s = S.sparse(k)
    n = len(s.src_p)
    R, e = counts(s, handoff=k <= 5)
    assert R["dims"] == (34, 34, 34) and abs(R["h"] - 0.5 * 1.1 ** 6) < 1e-9
    assert e["queued"] > 0.95 * n and e["queued_plain"] == e["queued"] == e["rest_searched"]
    assert (R["reason"][R["r1"] == S.PLAIN] == 1).all()                      # (the guard, not a query outside the grid)
    assert e["listed"] > 0.3 * n and e["queued"] - e["listed"] > 0.1 * n     # the lean 5x5x5 search finishes part and lists part
    assert e["queued"] * 4 > S.rest_blocks_one_pair(n) * S.REST_THREADS      # dense dealing
    assert int(np.ceil(s.r_p / R["h"])) + 1 == 4                             # the cooperative search's last shell (+ out)
    _, one = counts(s, one_stage=True, handoff=k <= 5)
    assert one["listed"] == one["exact"] == e["exact"] == 0                  # no exact ties among uniform points


def test_sparse_few_is_dealt_out():
    s = S.sparse_few()
    R, e = counts(s)
    assert R["dims"] == (24, 24, 24) and R["h"] == 0.5
    assert 40 <= e["queued"] <= 60 and e["listed"] >= 40
    assert e["queued"] * 4 <= S.rest_blocks_one_pair(len(s.src_p)) * S.REST_THREADS and e["listed"] * 4 <= S.rest_blocks_one_pair(len(s.src_p)) * S.REST_THREADS


@pytest.mark.parametrize("k", [3, 5, 6, 8, 9, 16])
def test_outside_populations(k):
    s = S.outside(k)
    R, e = counts(s)
    out = S.cell_out(s.src_p, R["origin"], R["h"], R["dims"])
    assert sorted(set(out.tolist())) == [0, 1, 2, 3, 4, 5, 9] and (np.bincount(out)[[0, 1, 2, 3, 4, 5, 9]] == 28).all()
    far = (out - 1) * R["h"] >= s.r_p
    assert (far == (out >= 6)).all()
    assert (R["r1"][far] == 0).all()                                         # count 0, not queued
    mid = (out > 1) & ~far
    assert (R["r1"][mid] == S.PLAIN).all() and mid.sum() == 4 * 28            # queued plain ...
    assert e["listed"] >= mid.sum() - 28                                      # ... and nearly all of them for the leftover kernel
    if k <= 5:
        assert (R["reason"][mid] == 3).all()                                  # (queued for lying outside, not on the guard)
    assert (R["r1"][out == 0] == 0).sum() >= 8                                # inside: round 1 finishes some at every k


def test_trip_budget_wide_from_64_batches():
    for n in (244, 248, 252, 256, 260):
        s = S.trip_budget(n)
        R, e = counts(s)
        out = S.cell_out(s.src_p, R["origin"], R["h"], R["dims"])
        assert R["h"] > 5.0 and (out == 0).all()
        cells = np.floor((s.tgt_p[:n] - R["origin"]) / R["h"])
        assert (cells == cells[0]).all() and (np.floor((s.src_p - R["origin"]) / R["h"]) == cells[0]).all()  # one cell holds cluster and queries
        wide = (n + 3) // 4 > 63
        assert (e["queued_wide"] == len(s.src_p)) == wide and (e["queued_wide"] == 0) == (not wide), (n, e)
        if wide:
            assert e["rest_searched"] == 0 and e["listed"] == e["queued"]            # two stages + coop: handed straight on
            assert counts(s, coop=False)[1]["rest_searched"] == e["queued"]           # NO_COOP_LEFT: the wide-number search
            assert counts(s, one_stage=True)[1]["rest_searched"] == e["queued"]


def test_lattice_ties():
    s5, s6 = S.lattice(5), S.lattice(6)
    n = len(s5.src_p)
    _, e5 = counts(s5, handoff=True)
    assert e5["late_min"] == e5["late"] == n and e5["queued_tied"] == 0 and e5["queued"] == 0
    _, e6 = counts(s6)
    assert e6["queued_tied"] == n and e6["rest_searched"] == 0 and e6["listed"] == n and e6["exact"] == n


def test_lattice_whose_ties_fp64_decides_still_ties_in_fp32():
    """the batch's lattice pair (queries 2^-30 .. 2^-28 m off their lattice points): the same late list as the exact lattice"""
    s = S.lattice(5, exact=False)
    n = len(s.src_p)
    _, e = counts(s, handoff=True)
    assert e["late_min"] == e["late"] == e["unverified"] == n and e["queued_tied"] == 0 and e["queued"] == 0  # late whatever the order in a cell
    d2 = ((s.tgt_p[None, :, :] - s.src_p[:20, None, :]) ** 2).sum(axis=2)
    d2.sort(axis=1)
    assert (np.diff(d2[:, :6], axis=1) > 0).all()  # FP64 orders the k + 1 nearest strictly (the hand-off's refusals above: FP32 cannot)


def test_lean_limit_twins():
    a, b = S.lean_limit(65536), S.lean_limit(65535)
    assert np.linalg.norm(a.src_p - a.tgt_p[65535], axis=1).min() > 2.0  # the point the twin lacks is beyond every query's radius
    assert np.array_equal(a.src_p, b.src_p) and len(a.tgt_p) == 65536 and len(b.tgt_p) == 65535
    (Ra, ea), (Rb, eb) = counts(a), counts(b)
    assert np.array_equal(Ra["r1"], Rb["r1"]) and ea["queued"] == ea["queued_plain"] > 50
    assert ea["rest_searched"] == 0 and ea["listed"] == ea["queued"]
    assert eb["rest_searched"] == eb["queued"] and 0 < eb["listed"] < eb["queued"]


@pytest.mark.parametrize("k", [2, 5, 8, 11])
def test_rod_is_beyond_the_cooperative_search(k):
    s = S.rod(k)
    R, e = counts(s)
    out = S.cell_out(s.src_e, R["origin"], R["h"], R["dims"])
    assert len(s.tgt_e) > S.K_BRUTE_MAX and R["dims"][0] > 64 and R["dims"][1:] == (1, 1)
    off = out > 1
    assert off.sum() == 100 and (R["r1"][off] == S.PLAIN).all() and (R["lean2"][off] < 0).all()
    assert (np.ceil(s.r_e / R["h"]) + 1 + out > S.K_COOP_MAX_SHELL).all() and (max(R["dims"]) + out > S.K_COOP_MAX_SHELL).all()
    assert e["listed"] >= 100 and e["exact"] == 0


def test_no_radius_has_a_queue():
    s = S.sparse(r=-1.0)
    R, e = counts(s, coop=False)
    assert R["dims"] == (8, 8, 8) and e["queued"] > 300 and e["listed"] > 100


def test_meet_fills_the_shared_list_exactly():
    s = S.meet()
    R, e = counts(s, handoff=True)
    assert len(s.src_p) == 2400 > len(s.tgt_p) == 2300
    assert e["listed"] > 300 and e["unverified"] > 1500 and e["listed"] + e["unverified"] == len(s.src_p)  # under FORCE_LATE_VERIFY: late = unverified


def test_brute_sizes():
    for n in S.BRUTE_SIZES:
        s = S.brute(n)
        assert len(s.tgt_e) == n <= S.K_BRUTE_MAX < len(s.tgt_p)
        if n >= 4:
            assert len(np.unique(s.tgt_e, axis=0)) < n  # duplicated points


def test_census_checks_accept_the_model_and_refuse_a_wrong_census():
    good = [S.model_census(S.trip_budget(256), False, False), S.model_census(S.sparse(), False, True), S.model_census(S.lattice(6), False, True),
            S.model_census(S.sparse(), True, False), S.model_census(S.wall(), False, True, handoff=True)]
    for c in good:
        S.check_census(c)
    wide, sparse = good[0], good[1]
    assert wide.queued_wide > 0 and sparse.listed > 0
    bad = copy.deepcopy(wide)      # a wide entry counted as tied
    bad.queued_wide -= 1
    bad.queued_tied += 1
    with pytest.raises(AssertionError):
        S.check_census(bad)
    bad = copy.deepcopy(wide)      # ... in its reason bits as well: rest_searched no longer fits them
    bad.queued_wide -= 1
    bad.queued_tied += 1
    bad.entry_reason[np.nonzero(bad.entry_reason & S.REASON_WIDE)[0][0]] = S.REASON_TIED
    with pytest.raises(AssertionError):
        S.check_census(bad)
    for d in (1, -1):              # a listed count off by one
        bad = copy.deepcopy(sparse)
        bad.listed += d
        bad.leftover_finished += d
        with pytest.raises(AssertionError):
            S.check_census(bad)
    bad = copy.deepcopy(sparse)    # exact above listed
    bad.exact = bad.listed + 1
    bad.leftover_finished = -1
    with pytest.raises(AssertionError):
        S.check_census(bad)
