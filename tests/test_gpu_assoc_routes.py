"""GPU: every route of the association's k-NN queue chain, asserted from the census of loamx_associate
(loamx_ctx_last_assoc_census). For every scene of tests/assoc_scenes.py and every form of the chain:
  1. the census has the form the scene was built for (launch form, search, KM, leftover kernel, dealing, lean set);
  2. its identities hold (assoc_scenes.check_census);
  3. its round-1 and queue counts EQUAL those of the g++ build of the kernels' own functions (tests/hostcheck) — the scenes
     leave no FP32 decision marginal that the two builds could take differently, so a difference is a finding, named per
     query from the census's per-entry arrays;
  4. lists in order and fits against the oracle (check_kind of tests/test_gpu_direct.py, its bars unchanged);
  5. every option set — QUEUE_ONE_STAGE, QUEUE_TWO_STAGE with and without NO_COOP_LEFT, FORCE_LATE_VERIFY, NO_MIXED_ASSOC,
     DEBUG_POISON — gives the default's dump (same_dump of tests/test_gpu_handoff.py; exact-tie scenes compare distances).
Then one batch of nine ragged pairs built from the scenes: every record equals the pair registered alone, the batch reversed
and the batch under QUEUE_ONE_STAGE, byte for byte. Each scene's census is printed once."""
import contextlib

import numpy as np
import pytest

import assoc_scenes as S
from gpu_common import ctx, option, pose_diff
from loam_amd import capi
from test_gpu_direct import check_kind
from test_gpu_handoff import same_dump

pytestmark = pytest.mark.gpu

OPTION_SETS = [("QUEUE_ONE_STAGE",), ("QUEUE_TWO_STAGE",), ("QUEUE_TWO_STAGE", "NO_COOP_LEFT"), ("NO_COOP_LEFT",), ("FORCE_LATE_VERIFY",),
               ("NO_MIXED_ASSOC",), ("DEBUG_POISON",)]
_printed = set()


def params(s, oracle):
    reg, oreg = capi.RegistrationParams(), oracle.RegParams()
    reg.num_edge_neighbors = oreg.num_edge_neighbors = s.k_e
    reg.num_plane_neighbors = oreg.num_plane_neighbors = s.k_p
    reg.max_edge_neighbor_dist = oreg.max_edge_neighbor_dist = s.r_e
    reg.max_plane_neighbor_dist = oreg.max_plane_neighbor_dist = s.r_p
    return reg, oreg


def associate(s, reg, opts=()):
    """(dump, census of the scene's kind, census of the other kind) under the option set"""
    with contextlib.ExitStack() as stack:
        for o in opts:
            stack.enter_context(option(o))
        dump = ctx().associate(s.src_e, s.src_p, s.tgt_e, s.tgt_p, S.IDENT, reg)
        cen = ctx().last_assoc_census(s.kind)
        other = ctx().last_assoc_census("edge" if s.kind == "plane" else "plane")
    if (s.name, opts) not in _printed:
        _printed.add((s.name, opts))
        print("census %s k=%d %s: %s" % (s.name, S.sets(s)[2], "+".join(opts) or "default",
                                         " ".join("%s=%s" % (n, getattr(cen, n)) for n in capi.ASSOC_CENSUS_SCALARS)))
    return dump, cen, other


def same_or_tied(s, a, b):
    """same_dump; a scene of exact ties compares the neighbours' distances instead of their indices (as the cooperative test
    of tests/test_gpu_direct.py does), for the kind the ties are in"""
    if not s.ties:
        return same_dump(a, b)
    q, t, k, r = S.sets(s)
    for kind in ("edge", "plane"):
        assert np.array_equal(a[kind]["valid"], b[kind]["valid"]) and np.array_equal(a[kind]["moved"], b[kind]["moved"])
        if kind != s.kind:
            assert all(np.array_equal(x, y) for x, y in zip(a[kind]["nn"], b[kind]["nn"])) and np.array_equal(a[kind]["prim"], b[kind]["prim"])
            continue
        for i, (x, y) in enumerate(zip(a[kind]["nn"], b[kind]["nn"])):
            assert len(x) == len(y) and np.array_equal(((t[x] - q[i]) ** 2).sum(axis=1), ((t[y] - q[i]) ** 2).sum(axis=1)), (kind, i)


def form_of(opts, s, mixed_possible):
    """(one_stage, leftover kernel, mixed launch) the launcher must report under the option set — queue_one_stage and
    queue_leftovers_coop spelled out for ONE pair far below kQueueTwoStageMin"""
    q, t, k, r = S.sets(s)
    no_coop = "NO_COOP_LEFT" in opts
    one = "QUEUE_TWO_STAGE" not in opts and ("QUEUE_ONE_STAGE" in opts or no_coop)
    left = capi.ASSOC_LEFTOVER_NONE if one else (capi.ASSOC_LEFTOVER_COOP if (not no_coop and r > 0) else capi.ASSOC_LEFTOVER_LEFT)
    return int(one), left, int(mixed_possible and "NO_MIXED_ASSOC" not in opts)


def diff_entries(cen, R, e):
    """which queries' entries differ from the g++ build's (for the failure message)"""
    want = np.nonzero(e["_queued"])[0]
    got = np.sort(cen.entry_query)
    return dict(only_gpu=np.setdiff1d(got, want)[:10], only_host=np.setdiff1d(want, got)[:10])


def walk(oracle, s, min_checked=0):
    """steps 1 - 5 of the module's docstring for a grid-searched scene"""
    q, t, k, r = S.sets(s)
    reg, oreg = params(s, oracle)
    plane = s.kind == "plane"
    mixed_possible = len(s.src_e) > 0 and len(s.src_p) > 0 and len(s.tgt_e) <= S.K_BRUTE_MAX < len(s.tgt_p) and s.k_e <= 5 and s.k_p <= 5
    first = None
    for opts in [()] + OPTION_SETS:
        dump, cen, other = associate(s, reg, opts)
        one, left, mixed = form_of(opts, s, mixed_possible)
        # 1. the form
        assert (cen.n_src, cen.n_tgt, cen.stride, cen.km) == (len(q), len(t), max(len(q), len(t)), S.km_of(k)), (s.name, opts)
        assert cen.search == capi.ASSOC_SEARCH_GRID and cen.n_points == len(t) and cen.lean_set == int(len(t) <= S.K_LEAN_MAX)
        assert (cen.one_stage, cen.leftover_kernel, cen.mixed_launch) == (one, left, mixed), (s.name, opts, cen.one_stage, cen.leftover_kernel, cen.mixed_launch)
        assert cen.rest_blocks == S.rest_blocks_one_pair(len(q)) and cen.coop_blocks == (4096 if left == capi.ASSOC_LEFTOVER_COOP else 0)
        assert cen.rest_spread == int(cen.queued * 4 <= cen.rest_blocks * S.REST_THREADS)
        assert cen.left_spread == int(left == capi.ASSOC_LEFTOVER_LEFT and cen.listed * 4 <= cen.rest_blocks * S.REST_THREADS)
        # 2. the identities
        S.check_census(cen)
        S.check_census(other)
        # 3. the g++ build's counts: the hand-off form of round 1 where the mixed launch ran the plane side
        R = S.routes(s, handoff=bool(mixed and plane))
        assert (tuple(cen.origin), cen.h, (cen.nx, cen.ny, cen.nz)) == (tuple(R["origin"]), R["h"], R["dims"])
        e = S.expected(R, len(t), bool(one), left == capi.ASSOC_LEFTOVER_COOP)
        # the late list, query by query: every selection the g++ build refuses whatever the order of the tied keys, and only
        # selections (assoc_scenes.COUNTS: the rest depends on the order of the target points inside a cell); all under FORCE_LATE_VERIFY
        must, may = np.nonzero(R["unverified"] if "FORCE_LATE_VERIFY" in opts else R["refused_any_order"])[0], np.nonzero(R["unverified"])[0]
        assert np.isin(must, cen.late_query).all() and np.isin(cen.late_query, may).all(), (
            s.name, opts, "not late on the GPU", np.setdiff1d(must, cen.late_query), "late but no selection", np.setdiff1d(cen.late_query, may))
        got = {n: getattr(cen, n) for n in S.COUNTS}
        assert got == {n: e[n] for n in S.COUNTS}, (s.name, opts, diff_entries(cen, R, e))
        order = np.argsort(cen.entry_query)
        assert np.array_equal(cen.entry_query[order], np.nonzero(e["_queued"])[0])
        assert np.array_equal(cen.count_after_rest[order] < 0, e["_after_rest"] < 0) and np.array_equal(cen.count_before_fit[order] < 0, e["_before_fit"] < 0)
        # 4. the oracle, 5. the default's dump
        if first is None:
            first = dump
            assert check_kind(oracle, s.name + " " + s.kind, dump, q, t, S.IDENT, plane, oreg, ties=s.ties) >= min_checked
            if mixed_possible:
                check_kind(oracle, s.name + " edge", dump, s.src_e, s.tgt_e, S.IDENT, False, oreg)
        else:
            same_or_tied(s, first, dump)
    return associate(s, reg)[1]


def test_census_lifetime(oracle):
    c = capi.Context(0)
    try:
        with pytest.raises(capi.LoamxError):
            c.last_assoc_census(1)  # before any association dump
        s = S.wall()
        c.associate(s.src_e, s.src_p, s.tgt_e, s.tgt_p, S.IDENT)
        assert c.last_assoc_census(1).n_src == len(s.src_p) and c.last_assoc_census(0).n_src == len(s.src_e)
        assert c.lib.loamx_ctx_last_assoc_census(c.h, 1, None) == capi.ERR_BAD_PARAM
        with pytest.raises(capi.LoamxError):
            c.last_assoc_census(2)
        c.register_features(s.src_e, s.src_p, s.tgt_e, s.tgt_p)
        with pytest.raises(capi.LoamxError):
            c.last_assoc_census(1)  # a registration came after the dump
        c.associate(s.src_e, s.src_p, s.tgt_e, s.tgt_p, S.IDENT)
        c.registration_information(s.src_e, s.src_p, s.tgt_e, s.tgt_p, S.IDENT)
        with pytest.raises(capi.LoamxError):
            c.last_assoc_census(1)  # an information call came after the dump
        w, f = S.wall(mixed=False), S.sparse_few()
        c.associate(w.src_e, w.src_p, w.tgt_e, w.tgt_p, S.IDENT)
        c.associate(f.src_e, f.src_p, f.tgt_e, f.tgt_p, S.IDENT)  # a second dump replaces the census
        cen, edge = c.last_assoc_census(1), c.last_assoc_census(0)
        assert (cen.n_src, cen.n_tgt) == (len(f.src_p), len(f.tgt_p)) and cen.queued >= 40
        assert (edge.km, edge.search, edge.n_tgt, edge.n_points, edge.h, edge.nx) == (0, 0, 0, 0, 0.0, 0)  # a kind that was not launched
    finally:
        c.close()


def test_wall_leaves_the_chain_at_its_first_test(oracle):
    cen = walk(oracle, S.wall(), 600)
    assert cen.mixed_launch == 1 and cen.queued == 0 and cen.listed == 0 and cen.unverified == cen.n_src
    cen = walk(oracle, S.wall(mixed=False), 600)  # (no edge sets: the plane kernels alone verify their own lists)
    assert cen.mixed_launch == 0 and cen.queued <= 3 and cen.unverified == 0


@pytest.mark.parametrize("k", [3, 5, 6, 8, 9, 16])
def test_sparse_dense_dealing_and_the_cooperative_walk(oracle, k):
    cen = walk(oracle, S.sparse(k))
    assert cen.km == S.km_of(k) and cen.queued * 4 > cen.n_src and cen.rest_spread == 0  # more than a quarter queued
    assert cen.leftover_kernel == capi.ASSOC_LEFTOVER_COOP and cen.leftover_finished == cen.listed > 0.3 * cen.n_src
    assert int(np.ceil(2.0 / cen.h)) + 1 + 1 == 5 <= S.K_COOP_MAX_SHELL  # the cooperative search applies and walks to shell 5 at most


def test_sparse_in_the_mixed_launch(oracle):
    cen = walk(oracle, S.sparse(5, mixed=True))
    assert cen.mixed_launch == 1 and cen.queued > 0.95 * cen.n_src


def test_sparse_few_spread_dealing(oracle):
    s = S.sparse_few()
    cen = walk(oracle, s, 600)
    assert 40 <= cen.queued <= 60 and cen.rest_spread == 1
    reg, _ = params(s, oracle)
    left = associate(s, reg, ("QUEUE_TWO_STAGE", "NO_COOP_LEFT"))[1]
    assert left.leftover_kernel == capi.ASSOC_LEFTOVER_LEFT and left.listed >= 40 and left.left_spread == 1
    dense = associate(S.sparse(), params(S.sparse(), oracle)[0], ("QUEUE_TWO_STAGE", "NO_COOP_LEFT"))[1]
    assert dense.left_spread == 0 and dense.listed * 4 > dense.rest_blocks * S.REST_THREADS


@pytest.mark.parametrize("k", [3, 5, 6, 8, 9, 16])
def test_outside_populations_from_the_census_grid(oracle, k):
    s = S.outside(k)
    cen = walk(oracle, s)
    out = S.cell_out(s.src_p, cen.origin, cen.h, (cen.nx, cen.ny, cen.nz))
    far = (out - 1) * cen.h >= s.r_p
    mid = (out > 1) & ~far
    assert far.sum() == 28 and mid.sum() == 4 * 28
    R = S.routes(s, False)
    near_queued = int(((out <= 1) & (R["r1"] > 0)).sum())  # (inside or one cell off: round 1 searches, its guard decides)
    assert cen.queued == mid.sum() + near_queued and cen.queued_plain == cen.queued
    assert cen.verified == cen.n_src - cen.queued
    # the cooperative search applies to every queued query, and starts with out > 0 for the ones outside
    assert (np.ceil(s.r_p / cen.h) + 1 + out[mid] <= S.K_COOP_MAX_SHELL).all() and cen.leftover_finished == cen.listed >= 3 * 28


def test_trip_budget(oracle):
    wide_n = []
    for n in (244, 248, 252, 256, 260):
        s = S.trip_budget(n)
        cen = walk(oracle, s, 30)
        host_wide = int((S.routes(s, False)["r1"] == S.WIDE).sum())
        assert cen.queued_wide == host_wide and cen.queued_wide in (0, cen.n_src)
        if cen.queued_wide:
            wide_n.append(n)
            assert cen.rest_searched == 0 and cen.listed == cen.queued == cen.n_src  # two stages + coop: straight to the wavefronts
            reg, _ = params(s, oracle)
            for opts in (("QUEUE_TWO_STAGE", "NO_COOP_LEFT"), ("QUEUE_ONE_STAGE",)):
                alt = associate(s, reg, opts)[1]
                assert alt.rest_searched == alt.queued == cen.n_src and alt.listed * 4 < alt.queued  # the wide-number search, in the rest kernel
    assert wide_n == [256, 260]  # ceil(n / 4) > 63 batches


def test_lattice_late_list_and_exact_collector(oracle):
    cen = walk(oracle, S.lattice(5))
    assert cen.mixed_launch == 1 and cen.late > cen.n_src // 2 and cen.queued_tied == 0
    cen = walk(oracle, S.lattice(5, exact=False), 150)  # the batch's lattice pair: FP64 decides its ties, FP32 does not: the same late list
    assert cen.mixed_launch == 1 and cen.late == cen.n_src and cen.queued_tied == 0 and cen.queued == 0
    cen = walk(oracle, S.lattice(6))
    assert cen.km == 8 and cen.mixed_launch == 0 and cen.queued_tied == cen.n_src and cen.rest_searched == 0
    assert cen.listed == cen.queued_tied and cen.exact == cen.n_src


def test_lean_limit_twins(oracle):
    a, b = S.lean_limit(65536), S.lean_limit(65535)
    ca, cb = walk(oracle, a, 20), walk(oracle, b, 20)
    assert ca.lean_set == 0 and ca.queued_plain == ca.queued > 50 and ca.rest_searched == 0 and ca.listed == ca.queued
    assert cb.lean_set == 1 and cb.rest_searched == cb.queued == ca.queued and 0 < cb.listed < cb.queued
    da = ctx().associate(a.src_e, a.src_p, a.tgt_e, a.tgt_p, S.IDENT)
    db = ctx().associate(b.src_e, b.src_p, b.tgt_e, b.tgt_p, S.IDENT)
    assert not any(65535 in x for x in da["plane"]["nn"])  # (the one point the twin lacks lies beyond every query's radius)
    assert all(np.array_equal(x, y) for x, y in zip(da["plane"]["nn"], db["plane"]["nn"]))  # same queries, same lists
    assert np.array_equal(da["plane"]["valid"], db["plane"]["valid"]) and np.array_equal(da["plane"]["prim"], db["plane"]["prim"])


@pytest.mark.parametrize("k", [2, 5, 8, 11])
def test_rod_edge_chain_beyond_the_cooperative_search(oracle, k):
    s = S.rod(k)
    cen = walk(oracle, s)
    assert cen.km == S.km_of(k) and cen.search == capi.ASSOC_SEARCH_GRID and cen.n_tgt > S.K_BRUTE_MAX and cen.mixed_launch == 0
    assert cen.leftover_kernel == capi.ASSOC_LEFTOVER_COOP and cen.listed >= 100 and cen.leftover_finished == cen.listed
    out = S.cell_out(s.src_e, cen.origin, cen.h, (cen.nx, cen.ny, cen.nz))
    off = out > 1
    assert off.sum() == 100 and np.isin(np.nonzero(off)[0], cen.entry_query[cen.count_after_rest < 0]).all()  # queued and listed, each of them
    # not applicable: more shells than kCoopMaxShell, and a grid wider than that (the census's GridDesc, the radius, out)
    assert (np.ceil(s.r_e / cen.h) + 1 + out[off] > S.K_COOP_MAX_SHELL).all() and (max(cen.nx, cen.ny, cen.nz) + out[off] > S.K_COOP_MAX_SHELL).all()


def test_no_radius_takes_the_one_lane_kernel(oracle):
    s = S.sparse(r=-1.0)
    cen = walk(oracle, s)
    assert cen.one_stage == 0 and cen.leftover_kernel == capi.ASSOC_LEFTOVER_LEFT and cen.queued > 300 and cen.listed > 100


def test_leftover_list_and_late_list_meet(oracle):
    s = S.meet()
    walk(oracle, s, 1500)  # (FORCE_LATE_VERIFY among the option sets: the same dump as without)
    late = associate(s, params(s, oracle)[0], ("FORCE_LATE_VERIFY",))[1]
    assert late.mixed_launch == 1 and late.leftover_kernel == capi.ASSOC_LEFTOVER_COOP and late.listed > 300 and late.late > 1500
    assert late.listed + late.late == late.n_src == late.stride  # no slot of K.exact to spare


@pytest.mark.parametrize("n", S.BRUTE_SIZES)
def test_brute_force_sizes(oracle, n):
    for k in (5, 3, 8):
        s = S.brute(n, k)
        reg, oreg = params(s, oracle)
        first = None
        for opts in [()] + OPTION_SETS:
            dump, cen, plane = associate(s, reg, opts)
            assert cen.search == capi.ASSOC_SEARCH_BRUTE and cen.km == S.km_of(k) and (cen.n_src, cen.n_tgt) == (len(s.src_e), n)
            assert cen.mixed_launch == plane.mixed_launch == int(k <= 5 and "NO_MIXED_ASSOC" not in opts)
            assert cen.queued == cen.unverified == cen.rest_blocks == cen.leftover_kernel == 0 and cen.verified == cen.n_src
            S.check_census(cen)
            S.check_census(plane)
            if first is None:
                first = dump
                check_kind(oracle, "%s k=%d edge" % (s.name, k), dump, s.src_e, s.tgt_e, S.IDENT, False, oreg, ties=s.ties)
                assert dump["edge"]["valid"].sum() >= (20 if n >= 255 else 0) and max(len(x) for x in dump["edge"]["nn"]) == min(k, n)
            else:
                same_or_tied(s, first, dump)


def batch_dev(c, scenes, es, ps, reg):
    """the scenes as ONE call of loamx_register_features_batch_dev at capacities es / ps: result bytes [pair][64]"""
    P = len(scenes)
    bufs = []
    for k, stride in ((0, es), (1, ps), (2, es), (3, ps)):
        pts, cnt = np.zeros((P, stride, 3)), np.zeros(P, np.uint32)
        for p, sc in enumerate(scenes):
            a = (sc.src_e, sc.src_p, sc.tgt_e, sc.tgt_p)[k]
            pts[p, :len(a)], cnt[p] = a, len(a)
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


def test_batch_of_nine_ragged_pairs(oracle):
    """nine pairs (one more than a group of eight: the dense dealing, rest_blocks = 4096 / 9 and coop_blocks = 32768 / 9 run), a pair
    with nearly every query queued next to one with none. The lattice pair is the one whose ties FP64 decides (assoc_scenes.lattice,
    exact=False): with EXACT ties the oracle's lists are its tree's traversal order, a registration's iteration count follows the
    four of six equidistant neighbours picked, and the g++ build of the kernels' own math stops after 2 iterations where the
    oracle takes 3 — nothing a registration can be held to."""
    rod = S.rod()
    scenes = [S.wall(), S.sparse(), S.outside(), S.trip_budget(256), S.lattice(5, exact=False), rod._replace(src_p=S.wall().src_p, tgt_p=S.wall().tgt_p),
              S.sparse_few(), S.sparse(r=-1.0), S.wall()]
    es, ps = max(max(len(s.src_e), len(s.tgt_e)) for s in scenes), max(max(len(s.src_p), len(s.tgt_p)) for s in scenes)
    c, reg = ctx(), capi.RegistrationParams()
    whole = batch_dev(c, scenes, es, ps, reg)
    for p, s in enumerate(scenes):
        assert np.array_equal(batch_dev(c, [s], es, ps, reg)[0], whole[p]), (p, s.name)
    assert np.array_equal(batch_dev(c, scenes[::-1], es, ps, reg)[::-1], whole)
    with option("QUEUE_ONE_STAGE"):
        assert np.array_equal(batch_dev(c, scenes, es, ps, reg), whole)
    rec = whole.reshape(-1).view(capi.RESULT_DTYPE)
    for p, s in enumerate(scenes):
        po, to, io = oracle.register_features(s.src_e, s.src_p, s.tgt_e, s.tgt_p)
        assert (int(rec["termination"][p]), int(rec["iterations"][p])) == (to, io), (p, s.name)
        rot, trans = pose_diff(oracle, po, np.array(rec["pose"][p]))
        assert rot < 1e-5 and trans < 1e-5, (p, s.name, rot, trans)
