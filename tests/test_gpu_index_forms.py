"""GPU: the target index at every form of its builds and merges. Each scene of tests/index_scenes.py is ASSERTED
to have taken its form from the library's read-out (loamx_target_index_census: the build the launcher chose, LDS passes, scan
tiles, table size, last operation, counters), the structure itself — order, cell table, float copies with their pads, grid
choice — is checked by plain numpy against the points (tests/index_common.py; loamx_knn_search cannot see a wrong float copy
or pad, its complete FP64 search does not read them), and k-NN lists are held to the oracle's KD-tree. The same scenes pass
the same checker on the CPU build in tests/test_index_hostcheck.py."""
import numpy as np
import pytest

import hostcheck_lib as Hc
import index_common as X
import index_scenes as S
from gpu_common import ctx, option
from loam_amd import capi
from test_gpu_direct import IDENT, check_kind

pytestmark = pytest.mark.gpu

NONE = np.zeros((0, 3))
_trees = {}


def reg_for(radius=2.0):
    reg = capi.RegistrationParams()
    reg.max_plane_neighbor_dist = radius
    return reg


def options(opts):
    import contextlib
    st = contextlib.ExitStack()
    for name, value in opts:
        st.enter_context(option(name, value))
    return st


def tree_of(oracle, key, pts):
    if key not in _trees:
        _trees.clear()  # (one tree at a time: the map scenes share theirs)
        _trees[key] = oracle.KDTree(pts)
    return _trees[key]


def check_knn(oracle, idx, which, pts, q, radius, key, ties=False, others=()):
    """k = 5 with the default radius and k = 8 without one, against the oracle's tree (and `others`: indexes that must agree)"""
    c = ctx()
    if len(pts) == 0:
        for k, r in ((5, 2.0), (8, -1.0)):
            assert all(len(g) == 0 for g in c.knn_search(idx, which, q, k, r))
        return
    tree = tree_of(oracle, key, pts)
    for k, r in ((5, radius if radius > 0 else 2.0), (8, -1.0)):
        got = c.knn_search(idx, which, q, k, r)
        rest = [c.knn_search(o, which, q, k, r) for o in others]
        for i in range(len(q)):
            want = tree.knn(q[i], k, r)
            for lists in [got] + rest:
                g = lists[i]
                if np.array_equal(g, want.astype(np.uint32)):
                    continue
                assert ties and len(g) == len(want), (key, k, r, i, g, want)  # (equal distances: the same numbers in the same order)
                assert np.array_equal(((pts[g.astype(np.int64)] - q[i]) ** 2).sum(axis=1), ((pts[want.astype(np.int64)] - q[i]) ** 2).sum(axis=1)), (key, i)


def end_queries_hit_the_ends(idx, which, cen, q, ties):
    """queries 0 and 1 are copies of the points at the last and the first sorted position: found as the nearest neighbour"""
    if cen.n == 0 or ties:
        return
    got = ctx().knn_search(idx, which, q[:2], 1, -1.0)
    assert got[0][0] == cen.orig[-1] and got[1][0] == cen.orig[0], (got, cen.orig[-1], cen.orig[0])


def check_full_build(cen, pts, radius, build, table_entries, table_valid):
    n = len(pts)
    ncell = X.ncell_of(cen)
    assert (cen.n, cen.n_points, cen.build, cen.table_entries, cen.table_valid, cen.last_op) == (n, n, build, table_entries, table_valid, capi.INDEX_OP_FULL_BUILD), cen[:15]
    assert cen.capacity >= max(n, 1)
    assert cen.lds_passes == (0 if build == S.BIG else X.ceil_div(ncell, X.LDS_CELLS))
    assert cen.scan_tiles == (X.ceil_div(ncell, X.SCAN_TILE) if build == S.BIG else 0)
    X.check_index(cen, pts)
    X.check_grid_choice(cen, pts, radius, table_entries, Hc)
    if cen.table_valid:
        assert np.array_equal(cen.cell_start, X.recount(cen, pts))


@pytest.mark.parametrize("name", S.ALL_SCENES)
def test_build_scene(oracle, name):
    sc = S.scene(name)
    c = ctx()
    with options(sc.options):
        idx = c.target_index(NONE, sc.pts, reg_for(sc.radius))
        try:
            cen = c.target_index_census(idx, 1)
            check_full_build(cen, sc.pts, sc.radius, sc.build, sc.table_entries, sc.table_valid)
            assert (cen.full_builds, cen.merges) == (1, 0) and c.target_index_stats(idx) == (2, 0)
            ncell = X.ncell_of(cen)
            if sc.dims is not None:
                assert cen.dims == sc.dims
            if sc.lds_passes is not None and sc.build != S.BIG:
                assert cen.lds_passes == sc.lds_passes
            if sc.scan_tiles is not None and sc.build == S.BIG:
                assert cen.scan_tiles == sc.scan_tiles
            if name == "map_log2_21":
                assert cen.scan_tiles > X.TILES_PER_ROUND and ncell > 1 << 20  # the second round of gridbig_tile_scan_kernel ran
            if len(sc.cells):
                assert (np.diff(cen.cell_start.astype(np.int64))[list(sc.cells)] > 0).all()
            empty = c.target_index_census(idx, 0)  # the edge kind: an empty set through the same build
            check_full_build(empty, NONE, 1.0, S.SINGLE if ("NO_PACKED_GRID", 1) in sc.options else S.PACKED, 65536, 0)
            q = S.queries(name, cen.xyz if cen.n else NONE, sc.pts, 90 if len(sc.pts) > 100000 else 190)
            if cen.n:
                q[0], q[1] = cen.xyz[-1], cen.xyz[0]
            end_queries_hit_the_ends(idx, 1, cen, q, sc.ties)
            check_knn(oracle, idx, 1, sc.pts, q, sc.radius, ("scene", len(sc.pts), name if len(sc.pts) < 200001 else "map"), sc.ties)
            if name == "no_big_30000":  # ... and a registration against it under the poisoned workspace equals the default build's
                src = sc.pts[::7] + 0.01
                a = c.register_features_indexed(idx, NONE, src)
        finally:
            c.target_index_destroy(idx)
    if name == "no_big_30000":
        idx = c.target_index(NONE, sc.pts, reg_for(sc.radius))
        try:
            assert c.target_index_census(idx, 1, arrays=False).build == S.BIG
            b = c.register_features_indexed(idx, NONE, src)
            assert a[1:] == b[1:] and np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))
        finally:
            c.target_index_destroy(idx)


def test_census_errors_and_skipped_arrays():
    c = ctx()
    sc = S.scene("n513")
    idx = c.target_index(NONE, sc.pts)
    try:
        cen = c.target_index_census(idx, 1, arrays=False)
        assert cen.cell_start is None and cen.xyz is None and cen.n == 513 and cen.build == S.PACKED
        v = capi.IndexCensusStruct()
        assert c.lib.loamx_target_index_census(c.h, idx, 2, v) == capi.ERR_BAD_PARAM
        assert c.lib.loamx_target_index_census(c.h, idx, 1, None) == capi.ERR_BAD_PARAM
        assert c.lib.loamx_target_index_census(c.h, None, 1, v) == capi.ERR_BAD_PARAM
        small = np.zeros(4, dtype=np.uint32)
        v.cell_start, v.cell_start_cap = small.ctypes.data_as(type(v.cell_start)), 4  # too small: refused, nothing written past it
        assert c.lib.loamx_target_index_census(c.h, idx, 1, v) == capi.ERR_BAD_PARAM
    finally:
        c.target_index_destroy(idx)


def test_crop_leaves_a_map_sized_capacity_with_a_small_and_an_empty_set(oracle):
    """gridbig_* on a set a crop has left at 300 points, then at none, while the capacity (25 000) keeps the multi-workgroup build"""
    c = ctx()
    pts = S.lattice("crop", (41, 41, 21), 25000)
    edge = S.lattice("crop_e", (41, 41, 21), 900)
    src_p, src_e = pts[::9] + 0.01, edge[::3] + 0.01
    idx = c.target_index(edge, pts)
    try:
        assert c.target_index_census(idx, 1, arrays=False).build == S.BIG
        xs = np.sort(pts[:, 0])
        cut = 0.5 * (xs[299] + xs[300])
        kept_p, kept_e = pts[pts[:, 0] <= cut], edge[edge[:, 0] <= cut]
        assert len(kept_p) == 300
        builds = 2
        for lo, hi, want_p, want_e in (([-np.inf] * 3, [cut, np.inf, np.inf], kept_p, kept_e), ([1e6] * 3, [2e6] * 3, NONE, NONE)):
            removed = c.target_index_crop(idx, lo, hi)
            builds += (removed[0] > 0) + (removed[1] > 0)
            assert c.target_index_size(idx) == (len(want_e), len(want_p)) and c.target_index_stats(idx) == (builds, 0)
            cen = c.target_index_census(idx, 1)
            check_full_build(cen, want_p, 2.0, S.BIG, 65536, 1)  # (the capacity chooses the build; its table is written at any size)
            assert cen.capacity == 25000
            fresh = c.target_index(want_e, want_p)
            try:
                fc = c.target_index_census(fresh, 1)
                check_full_build(fc, want_p, 2.0, S.PACKED, 65536, 0)
                assert np.array_equal(X.bits(np.array([cen.h])), X.bits(np.array([fc.h]))) and cen.dims == fc.dims
                q = S.queries("crop", cen.xyz if cen.n else NONE, want_p, 60)
                check_knn(oracle, idx, 1, want_p, q, 2.0, ("crop", len(want_p)), others=(fresh,))
                a = c.register_features_indexed(idx, src_e, src_p)
                b = c.register_features_indexed(fresh, src_e, src_p)
                assert a[1:] == b[1:] and np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))
            finally:
                c.target_index_destroy(fresh)
    finally:
        c.target_index_destroy(idx)


@pytest.mark.parametrize("name", S.MERGE_SCENES)
def test_merge_scene(oracle, name):
    ms = S.merge_scene(name)
    c = ctx()
    log2 = dict(ms.options).get("MAP_CELLS_LOG2", 0)
    radius = (1.0, 2.0)
    with options(ms.options):
        idx = c.target_index(ms.base_e, ms.base_p)
        try:
            sets = [ms.base_e, ms.base_p]
            counts = [[1, 0], [1, 0]]  # per kind: full builds, merges
            n_build = [len(ms.base_e), len(ms.base_p)]
            for si, step in enumerate(ms.steps):
                before = [c.target_index_census(idx, k, arrays=False) for k in range(2)]
                c.target_index_insert(idx, step[0], step[1])
                sets = [np.concatenate([sets[k], step[k]]) for k in range(2)]
                fresh = None
                for k in range(2):
                    want = step[2][k]
                    cen = c.target_index_census(idx, k)
                    if want is None:
                        assert (cen.full_builds, cen.merges, cen.n) == (counts[k][0], counts[k][1], len(sets[k]))
                        continue
                    counts[k][0 if want == "build" else 1] += 1
                    assert (cen.full_builds, cen.merges) == tuple(counts[k]), (name, si, k, want, cen.full_builds, cen.merges)
                    if want == "build":
                        n_build[k] = len(sets[k])
                        table = S.map_table_entries(n_build[k], log2)
                        check_full_build(cen, sets[k], radius[k], S.BIG, table, 1)
                        continue
                    table = S.map_table_entries(n_build[k], log2)
                    assert (cen.last_op, cen.build, cen.table_entries, cen.table_valid) == (capi.INDEX_OP_MERGE, S.BIG, table, 1)
                    assert cen.scan_tiles == X.ceil_div(X.ncell_of(cen), X.SCAN_TILE)
                    X.check_desc_kept(before[k], cen)
                    X.check_index(cen, sets[k])
                    assert np.array_equal(cen.cell_start, X.recount(cen, sets[k]))
                    if fresh is None:
                        fresh = c.target_index(sets[0], sets[1])
                    q = S.queries(name + str(si), cen.xyz, sets[k], 90)
                    q[0], q[1] = cen.xyz[-1], cen.xyz[0]
                    end_queries_hit_the_ends(idx, k, cen, q, False)
                    check_knn(oracle, idx, k, sets[k], q, radius[k], ("merge", name, si, k), others=(fresh,))
                if fresh is not None:
                    c.target_index_destroy(fresh)
                assert c.target_index_stats(idx) == (counts[0][0] + counts[1][0], counts[0][1] + counts[1][1])
            cen = c.target_index_census(idx, 1, arrays=False)
            if name == "scan_table":
                assert cen.table_entries == 65536 and cen.n == 35001 and cen.merges == 2
            if name == "cross_200000":
                assert cen.table_entries == 1 << 18 and cen.last_op == capi.INDEX_OP_FULL_BUILD and cen.n == 201000
            if name == "map_second_round":  # more than 256 tiles: the second round of index_insert_tile_scan_kernel ran
                assert cen.table_entries == 1 << 21 and X.ceil_div(cen.table_entries + 1, X.SCAN_TILE) > X.TILES_PER_ROUND
                assert cen.scan_tiles > X.TILES_PER_ROUND and cen.last_op == capi.INDEX_OP_MERGE
        finally:
            c.target_index_destroy(idx)


@pytest.mark.parametrize("n", [65535, 65536, 65537])
def test_lean_boundary_through_the_queue_kernels(oracle, n):
    """kLeanMaxPoints = 65 535: up to it the queue's lean search carries positions as 16-bit halves. The structure first (the
    same points as a persistent index), then loamx_associate in both queue forms against the oracle, with queries next to
    the points at the last and the first sorted position."""
    rng = np.random.default_rng(n)
    c = ctx()
    tgt = S.LO + rng.random((n, 3)) * np.array([60.0, 60.0, 20.0])
    idx = c.target_index(NONE, tgt)
    try:
        cen = c.target_index_census(idx, 1)
        check_full_build(cen, tgt, 2.0, S.BIG, 65536, 1)
    finally:
        c.target_index_destroy(idx)
    src = np.concatenate([[cen.xyz[-1] + 0.01, cen.xyz[0] - 0.01], cen.xyz[-40:] + rng.normal(size=(40, 3)) * 0.05,
                          tgt[rng.integers(0, n, 2000)] + rng.normal(size=(2000, 3)) * 0.05, S.LO + rng.random((1000, 3)) * np.array([60.0, 60.0, 20.0])])
    src = np.ascontiguousarray(src)
    reg, oreg = capi.RegistrationParams(), oracle.RegParams()
    dumps = {}
    for stage in ("QUEUE_ONE_STAGE", "QUEUE_TWO_STAGE"):
        with option(stage):
            dumps[stage] = c.associate(NONE, src, NONE, tgt, IDENT, reg)
        assert dumps[stage]["plane"]["queued"][0] > 0, (stage, dumps[stage]["plane"]["queued"])  # (the queue kernels had work)
    assert dumps["QUEUE_ONE_STAGE"]["plane"]["nn"][0][0] == cen.orig[-1] and dumps["QUEUE_ONE_STAGE"]["plane"]["nn"][1][0] == cen.orig[0]
    assert check_kind(oracle, f"plane lean-{n}", dumps["QUEUE_ONE_STAGE"], src, tgt, IDENT, True, oreg) >= 0
    two = dumps["QUEUE_TWO_STAGE"]["plane"]
    one = dumps["QUEUE_ONE_STAGE"]["plane"]
    assert all(np.array_equal(a, b) for a, b in zip(one["nn"], two["nn"])) and np.array_equal(one["valid"], two["valid"])
    assert np.array_equal(one["prim"][one["valid"]].view(np.uint64), two["prim"][two["valid"]].view(np.uint64))


@pytest.mark.parametrize("n", [511, 512, 513])
def test_batch_path_brute_force_boundary(oracle, n):
    """kBruteMax = 512 on the batch path (small_sets_build_kernel + the brute-force search, nine position bits; no persistent
    index, so no read-back): target edge AND planar sets of n points, the wanted neighbour the LAST point of each set, with
    and without NO_SMALL_SETS; lists equal to the oracle's, fits to 1e-12 (check_kind of tests/test_gpu_direct.py)."""
    rng = np.random.default_rng(n)
    c = ctx()
    poles = rng.random((8, 2)) * 6.0  # eight noisy vertical poles: lines fit
    tgt_e = np.column_stack([poles[rng.integers(0, 8, n)] + 0.005 * rng.normal(size=(n, 2)), rng.random(n) * 3.0])
    tgt_p = np.column_stack([rng.random(n) * 6.0, rng.random(n) * 6.0, 0.02 * rng.normal(size=n)])  # a noisy floor: planes fit
    src_e = np.concatenate([[tgt_e[-1] + 0.002], tgt_e[rng.integers(0, n, 150)] + rng.normal(size=(150, 3)) * 0.02])
    src_p = np.concatenate([[tgt_p[-1] + 0.002], tgt_p[rng.integers(0, n, 300)] + rng.normal(size=(300, 3)) * 0.02])
    reg, oreg = capi.RegistrationParams(), oracle.RegParams()
    for small in (True, False):
        with option("NO_SMALL_SETS", 0 if small else 1):
            dump = c.associate(src_e, src_p, tgt_e, tgt_p, IDENT, reg)
        assert dump["edge"]["nn"][0][0] == n - 1 and dump["plane"]["nn"][0][0] == n - 1
        ne = check_kind(oracle, f"edge brute-{n}-{small}", dump, src_e, tgt_e, IDENT, False, oreg)
        npl = check_kind(oracle, f"plane brute-{n}-{small}", dump, src_p, tgt_p, IDENT, True, oreg)
        assert ne > 20 and npl > 100, (ne, npl)
