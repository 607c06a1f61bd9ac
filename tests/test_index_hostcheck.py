"""CPU-only: the scenes of tests/index_scenes.py and the structure checker of tests/index_common.py, without a GPU.
  - every scene has the cell count, LDS passes and scan tiles it is meant to have, by the g++ build of grid_choose — a scene
    that drifts off its form fails here, before the GPU run (tests/test_gpu_index_forms.py);
  - check_index passes on the hostcheck's own build of every scene (cell table + order + float copies);
  - check_index refuses a correct structure with any one of five defects."""
import numpy as np
import pytest

import hostcheck_lib as Hc
import index_common as X
import index_scenes as S


def host_build(sc):
    return Hc.build_grid(sc.pts, sc.radius, sc.table_entries)


@pytest.mark.parametrize("name", S.ALL_SCENES)
def test_scene_has_its_form_and_the_host_build_passes_the_checker(name):
    sc = S.scene(name)
    n = len(sc.pts)
    opts = dict(sc.options)
    # the form the capacity (= n at create) and the options ask for (loamx_internal.h: grid_small; register_kernels.hip: grid_big)
    want = S.PACKED if n <= S.SMALL_CAP and not opts.get("NO_PACKED_GRID") else (S.SINGLE if n <= S.SMALL_CAP or opts.get("NO_BIG_GRID") else S.BIG)
    assert sc.build == want
    assert sc.table_entries == S.map_table_entries(n, opts.get("MAP_CELLS_LOG2", 0))
    assert sc.table_valid == (1 if (sc.build == S.BIG or n > S.BRUTE_MAX) else 0)
    assert sc.ties or len(np.unique(sc.pts, axis=0)) == n  # (no equal points: neighbour lists without ties)
    g = host_build(sc)
    ncell = X.ncell_of(g)
    if sc.dims is not None:
        assert g["dims"] == sc.dims, (g["dims"], sc.dims)
    if sc.ncell is not None:
        assert ncell == sc.ncell
    if sc.radius > 0 and name not in ("sparse_cap", "heavy_cell") and ncell > 1 and n < 100000:
        assert g["h"] == sc.radius / 4  # neither dense nor capped: the corners alone fix the grid
    assert ncell <= min(sc.table_entries, max(16 * n, 4096))
    if sc.build != S.BIG:
        assert X.ceil_div(ncell, X.LDS_CELLS) == (sc.lds_passes if sc.lds_passes is not None else X.ceil_div(ncell, X.LDS_CELLS))
    elif sc.scan_tiles is not None:
        assert X.ceil_div(ncell, X.SCAN_TILE) == sc.scan_tiles
    if len(sc.cells):
        pop = np.diff(g["cell_start"].astype(np.int64))
        assert (pop[list(sc.cells)] > 0).all(), (sc.cells, pop[list(sc.cells)])
    X.check_index(g, sc.pts)
    X.check_grid_choice(g, sc.pts, sc.radius, sc.table_entries, Hc)
    assert np.array_equal(g["cell_start"], X.recount(g, sc.pts))


def test_scenes_sit_on_the_features_they_are_named_for():
    g = host_build(S.scene("sparse_cap"))
    assert g["h"] > 0.5 and X.ncell_of(g) <= 9600 < 61 * 61 * 21  # the h *= 1.1 loop ran against the sparse cap
    g = host_build(S.scene("heavy_cell"))
    pop = np.diff(g["cell_start"].astype(np.int64))
    c = int(np.argmax(pop))
    assert pop[c] == S.SMALL_CAP - 2 and g["cell_start"][c + 1] == S.SMALL_CAP - 1 and c + 1 < X.ncell_of(g)  # offsets up to n - 1 behind it
    g = host_build(S.scene("dense_cell"))
    assert np.diff(g["cell_start"].astype(np.int64))[1000] > 255
    for name in ("two_pass", "cells_65536"):
        assert X.ceil_div(X.ncell_of(host_build(S.scene(name))), X.LDS_CELLS) == 2
    assert X.ncell_of(host_build(S.scene("cells_32768"))) == X.LDS_CELLS
    g = host_build(S.scene("map_log2_21"))
    assert X.ncell_of(g) > 1 << 20 and X.ceil_div(X.ncell_of(g), X.SCAN_TILE) > X.TILES_PER_ROUND
    g = host_build(S.scene("n200001"))
    assert X.ceil_div(X.ncell_of(g), X.SCAN_TILE) <= X.TILES_PER_ROUND  # (the default table never reaches the second round here)
    for name, chunks in (("n24576", 6), ("n24577", 7), ("n20481", 6)):
        assert X.ceil_div(len(S.scene(name).pts), 4096) == chunks


@pytest.mark.parametrize("name", ["n513", "odd_top", "two_pass", "big_4097"])
@pytest.mark.parametrize("how", X.MUTATIONS)
def test_checker_refuses_each_defect(name, how):
    sc = S.scene(name)
    g = host_build(sc)
    X.check_index(g, sc.pts)
    with pytest.raises(AssertionError):
        X.check_index(X.mutate(g, how), sc.pts)


def insert_ws_bytes(cells, n_add):
    """index_insert_ws_bytes (register_kernels.hip), restated for the arithmetic next to the both_kinds scene"""
    return 16 + 4 * (2 * (cells + 1) + n_add + X.ceil_div(cells + 1, X.SCAN_TILE))


@pytest.mark.parametrize("name", S.MERGE_SCENES)
def test_merge_scenes(name):
    """every step meant to be a merge adds points that lie inside the grid of the kind's last full build (cells computed without
    the clip), stays below twice the size at that build and inside the capacity; the host build of every stage passes"""
    ms = S.merge_scene(name)
    log2 = dict(ms.options).get("MAP_CELLS_LOG2", 0)
    for k, radius in ((0, 1.0), (1, 2.0)):
        pts = (ms.base_e, ms.base_p)[k]
        cap, n_build, grid = len(pts), len(pts), None
        for step in ms.steps:
            add, want = step[k], step[2][k]
            if want is None:
                assert len(add) == 0
                continue
            new = np.concatenate([pts, add])
            table = S.map_table_entries(n_build, log2)
            if want == "merge":
                assert grid is not None and n_build > S.SMALL_CAP and len(new) <= cap and len(new) <= 2 * n_build
                assert (len(new) > 200000) == (table > 65536)
                ijk = np.floor((add - grid["origin"]) * grid["inv_h"])
                assert (ijk >= 0).all() and (ijk < np.array(grid["dims"])).all()
                assert X.recount(grid, new)[-1] == len(new)
            else:
                while cap < len(new):
                    cap *= 2
                n_build = len(new)
                grid = Hc.build_grid(new, radius, S.map_table_entries(n_build, log2))
                X.check_index(grid, new)
            pts = new
    if name == "both_kinds":
        scratch = 64 + 4 * (65536 + 16 + 8)
        edge, planar = insert_ws_bytes(65536, 3000), insert_ws_bytes(65536, 6000)
        assert (edge, planar) == (536380, 548380) and edge > scratch
        off = (edge + 255) & ~255
        assert off == 536576 and off + planar > 2 * edge  # the planar part does not fit behind the edge part: the re-count path
    if name == "cross_200000":
        assert len(ms.base_p) + len(ms.steps[0][1]) == 198000 and len(ms.steps[1][1]) == 3000
    if name == "map_second_round":
        g = Hc.build_grid(np.concatenate([ms.base_p, ms.steps[0][1]]), 2.0, 1 << 21)
        assert X.ceil_div(X.ncell_of(g) + 1, X.SCAN_TILE) > X.TILES_PER_ROUND
