"""GPU: the listed leftovers of the queue chain by rows of lanes (associate_knn_coop_kernel since round 11) against
the same kernel with one wavefront per entry (context option NO_COOP_ROWS). Through loamx_associate and
loamx_ctx_last_assoc_census: neighbour lists, counts, flags, fits and every census field must be equal between the two forms, for
the scenes of tests/assoc_scenes.py that list entries (what the lists must BE — the oracle's, the g++ build's census — is asserted
for the default form by tests/test_gpu_assoc_routes.py), for pairs that list exactly 1, 4, 5, 64 and 65 entries (fewer entries
than a wavefront has rows, one more than it has, more than a wavefront of lanes), for a map-sized target, whose entries all keep
the wavefront, for `meet` with and without FORCE_LATE_VERIFY, and for a lean set that lists plain next to wide or tied entries.

Which form an entry took is counted by the kernel itself where it stores the entry's result, during an association dump only
(loamx_ctx_last_assoc_coop_forms: entries a row took, entries a wavefront took — no census field). both_forms asserts it for
every scene: by default the listed entries with plain reason bits of a lean set took a row and every other listed entry the
wavefront; under NO_COOP_ROWS none took a row. A kernel that never took its row branch fails every test here that lists a
plain entry against a lean set.

The deal beyond the first turn: a pair's second turn begins behind 4 x coop_blocks entries, and an association dump launches
4 096 workgroups for its one pair. test_the_second_turn_of_a_batch registers 512 pairs at once (coop_blocks = 64: 256 rows per
pair) with `sparse` (more than 360 listed entries) and `mixed_reasons` among them, by rows, by wavefronts and each pair alone.
tests/test_coop_rows_hostcheck.py models the deal itself on the host."""
import contextlib

import numpy as np
import pytest

import assoc_scenes as S
import index_scenes as I
from gpu_common import ctx, option
from loam_amd import capi
from test_gpu_handoff import same_dump

pytestmark = pytest.mark.gpu

ARRAYS = ("entry_reason", "count_after_rest", "count_before_fit")


def params(s):
    reg = capi.RegistrationParams()
    reg.num_edge_neighbors, reg.num_plane_neighbors = s.k_e, s.k_p
    reg.max_edge_neighbor_dist, reg.max_plane_neighbor_dist = s.r_e, s.r_p
    return reg


def same_census(a, b):
    """every scalar; the per-entry arrays by query (the queue's order is its atomics')"""
    for n in capi.ASSOC_CENSUS_SCALARS:
        assert getattr(a, n) == getattr(b, n), (n, getattr(a, n), getattr(b, n))
    oa, ob = np.argsort(a.entry_query), np.argsort(b.entry_query)
    assert np.array_equal(a.entry_query[oa], b.entry_query[ob])
    for n in ARRAYS:
        assert np.array_equal(getattr(a, n)[oa], getattr(b, n)[ob]), n
    assert np.array_equal(np.sort(a.late_query), np.sort(b.late_query))


def plain_listed(cen):
    """listed entries with plain reason bits: the ones a row takes when the set is lean"""
    return int(((cen.count_after_rest < 0) & ((cen.entry_reason & (S.REASON_WIDE | S.REASON_TIED)) == 0)).sum())


def associate(s, opts=()):
    """(dump, census, (entries a row took, entries a wavefront took)) of the scene's kind under the option set"""
    with contextlib.ExitStack() as stack:
        for o in opts:
            stack.enter_context(option(o))
        dump = ctx().associate(s.src_e, s.src_p, s.tgt_e, s.tgt_p, S.IDENT, params(s))
        return dump, ctx().last_assoc_census(s.kind), ctx().last_assoc_coop_forms(s.kind)


def both_forms(s, opts=()):
    """the scene in the default form and under NO_COOP_ROWS: the same dump, the same census, and the kernel's own count of the
    entries each form took; returns the default's dump and census"""
    dump, cen, forms = associate(s, opts)
    S.check_census(cen)
    wave_dump, wave_cen, wave_forms = associate(s, opts + ("NO_COOP_ROWS",))
    same_dump(dump, wave_dump)
    same_census(cen, wave_cen)
    coop = cen.leftover_kernel == capi.ASSOC_LEFTOVER_COOP
    rows = plain_listed(cen) if (coop and cen.lean_set) else 0
    assert forms == (rows, cen.listed - rows if coop else 0), (s.name, opts, forms, rows, cen.listed)
    assert wave_forms == (0, cen.listed if coop else 0), (s.name, opts, wave_forms, cen.listed)
    print("%s k=%d: listed %d (plain %d, exact %d), lean_set %d, leftover kernel %d" % (s.name, S.sets(s)[2], cen.listed, plain_listed(cen), cen.exact,
                                                                                        cen.lean_set, cen.leftover_kernel))
    return dump, cen


def test_the_option_is_off_by_default():
    assert ctx().get_option("NO_COOP_ROWS") == 0
    with option("NO_COOP_ROWS"):
        assert ctx().get_option("NO_COOP_ROWS") == 1
    assert ctx().get_option("NO_COOP_ROWS") == 0


@pytest.mark.parametrize("k", [3, 5, 6, 8, 9, 16])
def test_sparse_rows_equal_wavefronts(k):
    dump, cen = both_forms(S.sparse(k))
    # isolated queries of a lean set, plain reason bits, the cooperative kernel: every listed entry is a row's
    assert cen.leftover_kernel == capi.ASSOC_LEFTOVER_COOP and cen.lean_set == 1 and cen.coop_blocks == 4096
    assert plain_listed(cen) == cen.listed > 0.3 * cen.n_src and cen.leftover_finished == cen.listed


def test_sparse_few_outside_and_meet():
    _, cen = both_forms(S.sparse_few())
    assert cen.lean_set == 1 and plain_listed(cen) == cen.listed > 0
    _, cen = both_forms(S.outside())  # (rows whose queries start out = 2 .. 5 cells off the grid, next to rows that start inside)
    assert cen.lean_set == 1 and plain_listed(cen) == cen.listed >= 3 * 28
    _, cen = both_forms(S.meet())
    assert cen.mixed_launch == 1 and plain_listed(cen) == cen.listed > 0
    _, cen = both_forms(S.meet(), ("FORCE_LATE_VERIFY",))  # the leftover list and the late list meet in K.exact
    assert cen.mixed_launch == 1 and cen.listed + cen.late == cen.n_src == cen.stride and plain_listed(cen) == cen.listed > 0


def test_entries_that_keep_the_wavefront():
    _, cen = both_forms(S.trip_budget(256))  # wide entries: a dense block
    assert cen.lean_set == 1 and cen.queued_wide == cen.listed == cen.n_src and plain_listed(cen) == 0
    _, cen = both_forms(S.lattice(6))  # tied entries
    assert cen.queued_tied == cen.listed == cen.n_src and plain_listed(cen) == 0 and cen.exact == cen.n_src
    a, ca = both_forms(S.lean_limit(65536))  # one point more than a lean set: plain entries, but the wavefront's
    b, cb = both_forms(S.lean_limit(65535))  # its lean twin: rows
    assert ca.lean_set == 0 and plain_listed(ca) == ca.listed == ca.queued > 50
    assert cb.lean_set == 1 and 0 < plain_listed(cb) == cb.listed < cb.queued
    assert all(np.array_equal(x, y) for x, y in zip(a["plane"]["nn"], b["plane"]["nn"]))  # (the twins' lists are the same: the wavefront's and the rows')


def test_searches_the_cooperative_form_does_not_apply_to():
    _, cen = both_forms(S.rod())  # more than 64 shells: -2, the first lane of the row alone
    assert cen.leftover_kernel == capi.ASSOC_LEFTOVER_COOP and cen.lean_set == 1 and plain_listed(cen) == cen.listed >= 100
    _, cen = both_forms(S.sparse(5, r=0.0))  # no radius: the one-lane kernel takes the list
    assert cen.leftover_kernel == capi.ASSOC_LEFTOVER_LEFT


@pytest.fixture(scope="module")
def sparse_listed():
    """the queries of `sparse` by what became of them: listed, and finished by the rest kernel"""
    s = S.sparse()
    _, cen, _ = associate(s)
    return s, cen.entry_query[cen.count_after_rest < 0], cen.entry_query[cen.count_after_rest >= 0]


@pytest.mark.parametrize("n", [1, 4, 5, 64, 65])
def test_a_pair_that_lists_n_entries(sparse_listed, n):
    """n of the listed queries of `sparse` and 64 of the others against the same target (the pose is the identity: a query's route does
    not depend on the other queries): the pair lists exactly n — 1: three rows of the first wavefront idle; 4: one wavefront's rows;
    5: a second wavefront; 64 / 65: sixteen wavefronts and one row of the seventeenth. Against the wavefront form and the one-lane
    kernel, and every list against the full scene's"""
    s, listed, finished = sparse_listed
    pick = np.concatenate([np.sort(listed)[:n], np.sort(finished)[:64]])
    sub = s._replace(name="sparse_listed_%d" % n, src_p=np.ascontiguousarray(s.src_p[pick]))
    dump, cen = both_forms(sub)
    assert cen.listed == plain_listed(cen) == n and cen.lean_set == 1 and cen.coop_blocks == 4096
    one_lane, _, _ = associate(sub, ("QUEUE_TWO_STAGE", "NO_COOP_LEFT"))
    same_dump(dump, one_lane)
    full, _, _ = associate(s)
    for j, i in enumerate(pick):
        assert np.array_equal(dump["plane"]["nn"][j], full["plane"]["nn"][i]), (j, i)


def test_a_map_sized_target_keeps_the_wavefront():
    """200 000 points (index_scenes n200000: 100 x 100 x 30 m, not a lean set) and 300 queries up to 3 m above its top face:
    those a cell or two off the grid are queued and, in a map-sized set, listed without a search: all of them the wavefront's"""
    tgt = I.scene("n200000").pts
    rng = np.random.default_rng(121)
    src = I.LO + rng.random((300, 3)) * np.array([100.0, 100.0, 0.0]) + np.array([0.0, 0.0, 30.0]) + np.column_stack([np.zeros((300, 2)), rng.uniform(0.2, 3.0, 300)])
    s = S.scene("map_sized", "plane", S.NONE, src, S.NONE, tgt)
    dump, cen = both_forms(s)
    assert cen.lean_set == 0 and cen.leftover_kernel == capi.ASSOC_LEFTOVER_COOP and cen.rest_searched == 0 and cen.listed == cen.queued > 20
    one_lane, _, _ = associate(s, ("QUEUE_TWO_STAGE", "NO_COOP_LEFT"))
    same_dump(dump, one_lane)


def mixed_reasons():
    """the target of `sparse` with a cluster of 300 points in a cube of 0.1 m inside it (as `trip_budget`: more than 63 batches of four
    in one block, so round 1 runs out of running numbers) and the queries of `sparse` shuffled with 40 queries inside the cluster: a
    lean set whose list holds plain entries (isolated queries) next to wide ones (a dense block) — four of them in a wavefront's
    turn, in the order the rest kernel's atomics listed them. No ties: every decision is the same from run to run"""
    rng = np.random.default_rng(122)
    a = S.sparse()
    cluster = rng.uniform(-0.05, 0.05, (300, 3)) + np.array([3.0, -2.0, 1.0])
    inside = cluster[rng.choice(300, 40, replace=False)] + rng.normal(size=(40, 3)) * 0.003
    src = np.concatenate([a.src_p, inside])[rng.permutation(len(a.src_p) + 40)]
    return S.scene("mixed_reasons", "plane", S.NONE, src, S.NONE, np.concatenate([a.tgt_p, cluster]))


def test_plain_and_wavefront_entries_in_one_list():
    s = mixed_reasons()
    dump, cen = both_forms(s)  # (asserts rows == the plain listed entries, wavefronts == the others)
    assert cen.lean_set == 1 and plain_listed(cen) > 300 and cen.listed - plain_listed(cen) == cen.queued_wide == 40
    one_lane, _, _ = associate(s, ("QUEUE_TWO_STAGE", "NO_COOP_LEFT"))
    same_dump(dump, one_lane)


def test_the_second_turn_of_a_batch():
    """512 pairs in one call: coop_blocks = 32768 / 512 = 64 workgroups, 256 rows per pair. `sparse` and `mixed_reasons` list more than
    256 entries each (asserted from their dumps' censuses: the routes of a query do not depend on the batch), so their workgroups
    take a second turn — after their rows went their own ways in the first. Every record must equal the batch under NO_COOP_ROWS
    and the pair registered alone (4 096 workgroups: one turn), byte for byte"""
    from test_gpu_assoc_routes import batch_dev
    a, b, w = S.sparse(), mixed_reasons(), S.wall()
    assert associate(a)[1].listed > 256 and associate(b)[1].listed > 0
    print("listed: sparse %d, mixed_reasons %d" % (associate(a)[1].listed, associate(b)[1].listed))
    scenes = [w] * 512
    scenes[3], scenes[200], scenes[511] = a, b, a
    es, ps = max(max(len(s.src_e), len(s.tgt_e)) for s in scenes), max(max(len(s.src_p), len(s.tgt_p)) for s in scenes)
    c, reg = ctx(), capi.RegistrationParams()
    whole = batch_dev(c, scenes, es, ps, reg)
    with option("NO_COOP_ROWS"):
        assert np.array_equal(batch_dev(c, scenes, es, ps, reg), whole)
    for p in (0, 3, 200, 511):
        assert np.array_equal(batch_dev(c, [scenes[p]], es, ps, reg)[0], whole[p]), p
