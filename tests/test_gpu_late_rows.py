"""GPU: the late list of the plane fit searched by rows of 16 lanes (associate_fit_late_kernel, reg_math.h
knn_exact_block_row16). Every scene of tests/late_rows_scenes.py goes through loamx_associate in the mixed launch
(a small edge pair beside a planar target of more than 512 points, k <= 5) under FORCE_LATE_VERIFY, so that every selection
round 1 hands to the fit takes the late list. Per scene, in this order:
  1. the census reports late == unverified, equal to the count of the g++ build of the kernels' functions AND to the number the
     scene was built for, and the late list holds exactly those queries;
  2. lists, in order, and fits against the oracle (check_kind of tests/test_gpu_direct.py, its bars unchanged);
  3. the dump equals the dump without the option (same_dump of tests/test_gpu_handoff.py).
Scenes: list lengths around the rows of one pass (0, 1, 3, 4, 5, rows_per_pass - 1 / + 0 / + 1, three passes); blocks of 0, 1 .. 4,
15, 16, 17, 33 and 244 - 252 candidates and one above the row's 256 (the one-lane search of lane 0); k = 1 .. 5; corner cells and
queries one cell outside the grid on every side; a coplanar target; exact ties (the lattice, duplicated points); neighbours
within 1e-9 of the radius on either side (kept = 0 .. k). Then nine ragged pairs as one batch of registrations: byte for byte
against each pair alone and the batch reversed, with and without FORCE_LATE_VERIFY, and again under DEBUG_POISON.

The completeness fallback (a block whose k best do not pass knn_done's test at w = 1) cannot be reached from the late list:
a query is only on it when round 1 made a selection, and round 1 selects only behind the same test taken with the rigorous
bound — the FP32 k-th distance plus its error, never below the exact one, against the same faces (reg_math.h: "same test as
knn_done, with the rigorous bound"). tests/test_late_rows_hostcheck.py reaches it on the host (case `sparse`); here the
one-lane search behind the row is covered by the scene above the row's capacity."""
import numpy as np
import pytest

import assoc_scenes as S
import late_rows_scenes as L
from gpu_common import ctx, option
from loam_amd import capi
from test_gpu_assoc_routes import associate, batch_dev, params
from test_gpu_direct import check_kind
from test_gpu_handoff import same_dump

pytestmark = pytest.mark.gpu

FORCE = ("FORCE_LATE_VERIFY",)


def walk(oracle, s, want_late):
    """steps 1 - 3 of the module's docstring -> (the dump under FORCE_LATE_VERIFY, its census)"""
    reg, oreg = params(s, oracle)
    assert len(s.src_e) > 0 and len(s.tgt_e) <= S.K_BRUTE_MAX < len(s.tgt_p) and s.k_e <= 5 and s.k_p <= 5  # the mixed launch
    plain, _, _ = associate(s, reg)
    dump, cen, _ = associate(s, reg, FORCE)
    R = S.routes(s, True)
    print("late %s: n_src %d late %d unverified %d queued %d rest_blocks %d" % (s.name, cen.n_src, cen.late, cen.unverified, cen.queued, cen.rest_blocks))
    # 1. the census
    assert cen.mixed_launch == 1 and cen.km == 5 and cen.rest_blocks == S.rest_blocks_one_pair(len(s.src_p)), s.name
    S.check_census(cen)
    assert cen.late == cen.unverified == int(R["unverified"].sum()) == want_late, (s.name, cen.late, cen.unverified, int(R["unverified"].sum()), want_late)
    assert np.array_equal(np.sort(cen.late_query), np.nonzero(R["unverified"])[0]), s.name
    # 2. the oracle
    check_kind(oracle, s.name + " plane", dump, s.src_p, s.tgt_p, S.IDENT, True, oreg, ties=s.ties)
    check_kind(oracle, s.name + " edge", dump, s.src_e, s.tgt_e, S.IDENT, False, oreg)
    # 3. the dump without the option
    same_dump(plain, dump)
    return dump, cen


@pytest.mark.parametrize("late", [0, 1, 3, 4, 5, 15, 16, 17, 48])
def test_list_lengths_around_a_pass_of_rows(oracle, late):
    s, want = L.list_length(late)
    assert L.rows_per_pass(len(s.src_p)) == 16  # 15, 16, 17: one short of a pass, a pass, one more; 48: three passes
    dump, cen = walk(oracle, s, want)
    assert [len(x) for x in dump["plane"]["nn"]] == [5] * late + [0] * (len(s.src_p) - late)


@pytest.mark.parametrize("m", [1, 2, 3, 4, 15, 16, 17, 33, 244, 248, 252])
def test_block_populations(oracle, m):
    s, want = L.block_population(m)
    dump, cen = walk(oracle, s, want)
    assert cen.h > 4.0 and want == len(s.src_p)  # the cluster alone in its block
    assert all(len(x) == min(m, 5) for x in dump["plane"]["nn"])  # (m < k: kept < k)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_fewer_neighbours_than_slots(oracle, k):
    s, want = L.block_population(33, k)
    dump, cen = walk(oracle, s, want)
    assert all(len(x) == k for x in dump["plane"]["nn"])


def test_empty_block(oracle):
    s, want = L.empty_block()
    dump, cen = walk(oracle, s, want)
    assert want == len(s.src_p) and all(len(x) == 0 for x in dump["plane"]["nn"]) and not dump["plane"]["valid"].any()


def test_block_above_the_rows_capacity_takes_the_one_lane_search(oracle):
    import hostcheck_lib as Hc
    h = Hc.grid_choose(L.over_capacity(5.0)[0].tgt_p, 2.0)[0]  # (the cell edge depends on the set's size and box alone)
    s, want = L.over_capacity(h)
    dump, cen = walk(oracle, s, want)
    assert cen.h == h and want == len(s.src_p)
    # 300 points in the block of every query, 150 on either side of the face between two of its rows
    cy = np.floor((s.tgt_p[:300, 1] - cen.origin[1]) / cen.h)
    assert (cy[:150] == cy[0]).all() and (cy[150:] == cy[0] + 1).all() and 300 > L.ROW_CAP
    assert (np.floor((s.src_p[:, 1] - cen.origin[1]) / cen.h) == cy[0]).all()
    assert all(len(x) == 5 for x in dump["plane"]["nn"])


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_neighbours_just_inside_and_outside_the_radius(oracle, k):
    s, want = L.radius_shells(k)
    dump, cen = walk(oracle, s, want)
    assert [len(x) for x in dump["plane"]["nn"]] == L.kept_of_radius_shells(k)  # kept = 0 .. k


def test_corner_cells_and_one_cell_outside_the_grid(oracle):
    s, out = L.box_edges()
    R = S.routes(s, True)
    want = int(R["unverified"].sum())
    # every corner-cell query and most of those outside are finished by round 1 (the others: the block's faces nearer than the fifth neighbour)
    assert R["unverified"][out == 0].all() and (out == 0).sum() == 8 and R["unverified"][out == 1].sum() >= 12 and (out <= 1).all()
    dump, cen = walk(oracle, s, want)
    sides = {(axis, side) for axis in range(3) for side in (-1, 1)}
    dims = np.array([cen.nx, cen.ny, cen.nz])
    cell = np.floor((s.src_p - cen.origin) / cen.h).astype(int)
    seen = {(axis, -1 if cell[i, axis] < 0 else 1) for i in cen.late_query for axis in range(3) if cell[i, axis] < 0 or cell[i, axis] >= dims[axis]}
    assert seen == sides  # a late query one cell outside on every side of the grid


def test_coplanar_target(oracle):
    s, want = L.flat()
    dump, cen = walk(oracle, s, want)
    assert cen.ny == 1 and want == len(s.src_p)
    cy = np.floor((s.src_p[:, 1] - cen.origin[1]) / cen.h)
    assert (cy == 0).sum() == (cy == -1).sum() == len(s.src_p) // 2  # half in the only layer, half one cell outside it


def test_exact_ties(oracle):
    for s in (S.lattice(5), S.lattice(5, exact=False)):
        R = S.routes(s, True)
        dump, cen = walk(oracle, s, int(R["unverified"].sum()))
        assert cen.late == cen.n_src and cen.queued == 0  # six equidistant neighbours around every query: (d2, orig) decides
    s, want = L.duplicates()
    dump, cen = walk(oracle, s, want)
    assert want == len(s.src_p)
    for x in dump["plane"]["nn"]:  # twins at equal distance come in the order of their original indices
        d = ((s.tgt_p[x] - s.tgt_p[x[0]]) ** 2).sum(axis=1)
        assert len(x) == 5 and all(x[j] < x[j + 1] for j in range(4) if np.array_equal(s.tgt_p[x[j]], s.tgt_p[x[j + 1]])), (x, d)


def test_batch_of_nine_ragged_pairs():
    import hostcheck_lib as Hc
    h = Hc.grid_choose(L.over_capacity(5.0)[0].tgt_p, 2.0)[0]
    scenes = [L.list_length(17)[0], L.block_population(33)[0], L.block_population(252)[0], L.over_capacity(h)[0], L.radius_shells(5)[0],
              L.box_edges()[0], L.flat()[0], S.lattice(5, exact=False), L.block_population(3)[0]]
    es, ps = max(max(len(s.src_e), len(s.tgt_e)) for s in scenes), max(max(len(s.src_p), len(s.tgt_p)) for s in scenes)
    c, reg = ctx(), capi.RegistrationParams()
    reg.min_associations = 10  # (the scenes have 6 - 60 planar queries and 45 edge queries each: registrations that run)
    whole = batch_dev(c, scenes, es, ps, reg)
    for poison in (False, True):
        with option("DEBUG_POISON", 1 if poison else 0):
            for force in (False, True):
                with option("FORCE_LATE_VERIFY", 1 if force else 0):
                    assert np.array_equal(batch_dev(c, scenes, es, ps, reg), whole), (poison, force)
                    for p, s in enumerate(scenes):
                        assert np.array_equal(batch_dev(c, [s], es, ps, reg)[0], whole[p]), (poison, force, p, s.name)
                    assert np.array_equal(batch_dev(c, scenes[::-1], es, ps, reg)[::-1], whole), (poison, force)
    rec = whole.reshape(-1).view(capi.RESULT_DTYPE)
    assert (rec["iterations"] >= 1).sum() >= 7, rec["iterations"]  # (association passes that ran, the late kernel behind each)
