"""Point sets that send the target index through every form of its builds and merges, each with the form it is
meant to have. tests/test_index_hostcheck.py asserts the forms from the CPU grid_choose and runs the structure checker on the
host build of every scene; tests/test_gpu_index_forms.py asserts them from the library's read-out (loamx_target_index_census).

Placement. Most scenes fix the grid by two box corners: with cell edge h the corners lo and lo + (dims - 0.5) h give
floor(e / h) + 1 = dims cells per axis, and the top corner lies in the last cell. h = radius / 4 holds while the set is not
"dense" (grid_choose: h_dense = sqrt(8 area / n) >= h, i.e. n <= 8 area / h^2), while nx ny nz fits the table and while it
fits the sparse cap max(16 n, 4096). The CPU leg checks that every scene sits where it is meant to."""
import collections

import numpy as np

PACKED, SINGLE, BIG = 1, 2, 3  # LOAMX_INDEX_BUILD_*
H = 0.5                        # cell edge at the default planar radius 2.0
LO = np.array([-3.25, 1.5, -0.75])
SMALL_CAP, BRUTE_MAX = 20480, 512

Scene = collections.namedtuple("Scene", "name pts radius options build dims ncell lds_passes scan_tiles table_entries table_valid ties cells")
# options: context options of the build; dims / ncell: None where the scene does not fix them; cells: cells that must be occupied
_cache = {}


def _rng(name):
    return np.random.default_rng(abs(hash_name(name)))


def hash_name(name):
    v = 1469598103934665603
    for ch in name.encode():
        v = ((v ^ ch) * 1099511628211) % (1 << 63)
    return v


def cell_centre(dims, cell, h=H, lo=LO):
    """a point inside cell `cell`, off its middle: the top corner of lattice() is the middle of the last cell, and two equal
    points would leave the order of a neighbour list to the tie rule"""
    ix, iy, iz = cell % dims[0], (cell // dims[0]) % dims[1], cell // (dims[0] * dims[1])
    return lo + (np.array([ix, iy, iz]) + 0.375) * h


def lattice(name, dims, n, cells=(), h=H, fill=None):
    """n points whose grid is `dims` cells of edge h: the two corners, one point inside every cell of `cells`, the
    rest uniform in the box (or in `fill` = (lo fraction, hi fraction) of it)"""
    rng = _rng(name)
    dims = np.array(dims)
    ext = (dims - 0.5) * h
    fixed = [LO, LO + ext] + [cell_centre(dims, c, h) for c in cells]
    f_lo, f_hi = fill if fill is not None else (np.zeros(3), np.ones(3))
    u = LO + (np.asarray(f_lo) + rng.random((n - len(fixed), 3)) * (np.asarray(f_hi) - np.asarray(f_lo))) * ext
    return np.concatenate([np.array(fixed), u])


def uniform(name, n, box):
    rng = _rng(name)
    return LO + rng.random((n, 3)) * np.array(box)


def _scene(name, pts, build, radius=2.0, options=(), dims=None, ncell=None, passes=None, tiles=0, table=65536, valid=1, ties=False, cells=()):
    if dims is not None:
        ncell = int(np.prod(dims))
    if passes is None and build != BIG and ncell is not None:
        passes = -(-ncell // 32768)
    return Scene(name, np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3), radius, tuple(options), build, None if dims is None else tuple(dims),
                 ncell, 0 if build == BIG else passes, tiles, table, valid, ties, tuple(cells))


def _make(name):
    S = _scene
    NOPACK = (("NO_PACKED_GRID", 1),)
    # ---- packed single-workgroup build (capacity <= 20 480) ----
    if name == "n0":
        return S(name, np.zeros((0, 3)), PACKED, dims=(1, 1, 1), valid=0)
    if name == "n1":
        return S(name, LO[None] + 0.125, PACKED, dims=(1, 1, 1), valid=0)
    if name == "n512":
        return S(name, uniform(name, 512, (6, 6, 3)), PACKED, valid=0)
    if name == "n513":
        return S(name, uniform(name, 513, (6, 6, 3)), PACKED)
    if name == "n20480":
        return S(name, uniform(name, SMALL_CAP, (16, 16, 8)), PACKED)
    # (all points identical: at a positive x. The reference's KD-tree — nanoflann's middleSplit, copied by the oracle — cuts a box
    # of zero extent at 0; with the points on the negative side the empty leaf lies BEHIND the last point and its box is read
    # past the end of the index array, which is undefined in the reference itself)
    if name == "identical_radius":  # h = r / 4, one cell
        return S(name, np.tile(np.abs(LO) + 0.3, (600, 1)), PACKED, dims=(1, 1, 1), ties=True)
    if name == "identical_no_radius":  # area 0, no radius: h = 1
        return S(name, np.tile(np.abs(LO) + 0.3, (600, 1)), PACKED, radius=-1.0, dims=(1, 1, 1), ties=True)
    if name == "collinear":  # exactly on one axis: the area term is 0, h = r / 4; 81 cells (odd)
        p = np.tile(LO, (3000, 1))
        p[:, 0] += np.concatenate([[0.0, 40.25], _rng(name).random(2998) * 40.25])
        return S(name, p, PACKED, dims=(81, 1, 1))
    if name == "coplanar":  # a flat box: nz = 1
        p = lattice(name, (41, 41, 1), 5000)
        p[:, 2] = LO[2]
        return S(name, p, PACKED, dims=(41, 41, 1))
    if name == "odd_top":  # an odd cell count whose last cell (half of a packed word) is occupied
        return S(name, lattice(name, (15, 13, 11), 3000), PACKED, dims=(15, 13, 11), cells=(2144,))
    if name == "cells_32768":  # one pass exactly
        return S(name, lattice(name, (32, 32, 32), 4096, cells=(32767,)), PACKED, dims=(32, 32, 32), cells=(32767,))
    if name in ("two_pass", "two_pass_unpacked"):  # the second pass with its carry; both sides of the seam occupied
        return S(name, lattice("two_pass", (40, 40, 25), 4096, cells=(32767, 32768)), PACKED if name == "two_pass" else SINGLE,
                 options=() if name == "two_pass" else NOPACK, dims=(40, 40, 25), cells=(32767, 32768, 39999))
    if name in ("cells_65536", "cells_65536_unpacked"):  # cell 65 535 in a 16-bit value
        return S(name, lattice("cells_65536", (64, 64, 16), 4096, cells=(32767, 32768)), PACKED if name == "cells_65536" else SINGLE,
                 options=() if name == "cells_65536" else NOPACK, dims=(64, 64, 16), cells=(32767, 32768, 65535))
    if name == "sparse_cap":  # 61 x 61 x 21 cells at r / 4 against a cap of max(16 n, 4096) = 9 600: the h *= 1.1 loop runs
        return S(name, uniform(name, 600, (30, 30, 10)), PACKED)
    if name == "heavy_cell":  # n - 2 points in one cell: the largest offset a 16-bit half carries (20 479 behind it)
        p = np.concatenate([[LO, LO + 4.0], LO + 1.03 + (_rng(name).random((SMALL_CAP - 2, 3)) - 0.5) * 0.01])
        return S(name, p, PACKED)
    if name == "dense_cell":  # more than 255 points in a cell next to the queries (wide running numbers of the queue's search)
        base = lattice(name, (15, 13, 11), 4000)
        base[100:500] = cell_centre((15, 13, 11), 1000) + (_rng(name + "c").random((400, 3)) - 0.5) * 0.4
        return S(name, base, PACKED, dims=(15, 13, 11), cells=(1000,))
    # ---- unpacked single-workgroup build ----
    if name == "no_big_30000":
        return S(name, lattice(name, (41, 41, 21), 30000), SINGLE, options=(("NO_BIG_GRID", 1), ("DEBUG_POISON", 1)), dims=(41, 41, 21))
    # ---- multi-workgroup build (capacity > 20 480): chunks of 4 096 points, scan tiles of 4 096 entries ----
    if name == "n20481":
        return S(name, uniform(name, SMALL_CAP + 1, (16, 16, 8)), BIG, tiles=None)
    if name == "n24576":  # six chunks exactly
        return S(name, uniform(name, 24576, (16, 16, 8)), BIG, tiles=None)
    if name == "n24577":  # ... and one point more
        return S(name, uniform(name, 24577, (16, 16, 8)), BIG, tiles=None)
    if name == "big_4095":
        return S(name, lattice(name, (63, 65, 1), SMALL_CAP + 1, cells=(4094,)), BIG, dims=(63, 65, 1), tiles=1, cells=(4094,))
    if name == "big_4096":
        return S(name, lattice(name, (32, 64, 2), SMALL_CAP + 1, cells=(4095,)), BIG, dims=(32, 64, 2), tiles=1, cells=(4095,))
    if name == "big_4097":
        return S(name, lattice(name, (17, 241, 1), SMALL_CAP + 1, cells=(4095, 4096)), BIG, dims=(17, 241, 1), tiles=2, cells=(4095, 4096))
    if name == "big_65536":
        return S(name, lattice(name, (64, 64, 16), SMALL_CAP + 1, cells=(4095, 4096, 61439, 61440)), BIG, dims=(64, 64, 16), tiles=16,
                 cells=(4095, 4096, 61439, 61440, 65535))
    # ---- map tables (more than 200 000 points) ----
    if name == "n200000":
        return S(name, uniform("map", 200000, (100, 100, 30)), BIG, tiles=None)
    if name == "n200001":
        return S(name, uniform("map", 200001, (100, 100, 30)), BIG, tiles=None, table=1 << 18)
    if name == "map_log2_8":  # a 256-entry request is not honoured: the kind takes the scan-sized table
        return S(name, uniform("map", 200001, (100, 100, 30)), BIG, options=(("MAP_CELLS_LOG2", 8),), tiles=None)
    if name == "map_log2_17":
        return S(name, uniform("map", 200001, (100, 100, 30)), BIG, options=(("MAP_CELLS_LOG2", 17),), tiles=None, table=1 << 17)
    if name == "map_log2_21":  # more than 2^20 cells: more than 256 scan tiles, the second round of the tile-sum scan
        return S(name, uniform("map", 200001, (100, 100, 30)), BIG, options=(("MAP_CELLS_LOG2", 21),), tiles=None, table=1 << 21)
    raise KeyError(name)


PACKED_SCENES = ("n0", "n1", "n512", "n513", "n20480", "identical_radius", "identical_no_radius", "collinear", "coplanar", "odd_top",
                 "cells_32768", "two_pass", "cells_65536", "sparse_cap", "heavy_cell", "dense_cell")
SINGLE_SCENES = ("two_pass_unpacked", "cells_65536_unpacked", "no_big_30000")
BIG_SCENES = ("n20481", "n24576", "n24577", "big_4095", "big_4096", "big_4097", "big_65536")
MAP_SCENES = ("n200000", "n200001", "map_log2_8", "map_log2_17", "map_log2_21")
ALL_SCENES = PACKED_SCENES + SINGLE_SCENES + BIG_SCENES + MAP_SCENES


def scene(name):
    if name not in _cache:
        _cache[name] = _make(name)
    return _cache[name]


def queries(name, census_xyz, pts, n_random=190):
    """about 200 queries: jittered copies of points, points outside the box, and one query each whose nearest neighbour is the
    point at the LAST and at the FIRST sorted position (census_xyz: the cell-sorted points)"""
    rng = _rng(name + "/q")
    if len(pts) == 0:
        return rng.normal(size=(8, 3))
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    jit = pts[rng.integers(0, len(pts), n_random)] + rng.normal(size=(n_random, 3)) * 0.05
    outside = np.array([hi + 0.7, lo - 0.7, [hi[0] + 5.0, lo[1], lo[2]], (lo + hi) / 2 + [0, 0, (hi - lo)[2] + 1.0]])
    ends = np.array([census_xyz[-1] + 1e-5, census_xyz[0] - 1e-5])
    return np.concatenate([ends, jit, outside])


# ---- the merge scenes: base set, the inserts that follow, what each insert must be ---------------------------------
MergeScene = collections.namedtuple("MergeScene", "name options base_e base_p steps")
# steps: (edge points, planar points, expected op per kind: "merge" / "build" / None (untouched)), in order


def _inside(name, n, dims, fill=None):
    """n points strictly inside the box of lattice(dims)"""
    ext = (np.array(dims) - 0.5) * H
    f_lo, f_hi = fill if fill is not None else (np.zeros(3), np.ones(3))
    return LO + (np.asarray(f_lo) + _rng(name).random((n, 3)) * (np.asarray(f_hi) - np.asarray(f_lo))) * ext


def merge_scene(name):
    none = np.zeros((0, 3))
    M = MergeScene
    if name == "scan_table":  # 30 000 + 5 000 into the 65 536-entry table (the first insert outgrows the exact capacity: a rebuild)
        d = (41, 41, 21)
        return M(name, (), none, lattice(name, d, 29000), [(none, _inside(name + "1", 1000, d), (None, "build")),
                                                           (none, _inside(name + "2", 5000, d), (None, "merge")),
                                                           (none, _inside(name + "3", 1, d), (None, "merge"))])
    if name == "empty_and_last_cells":  # the base leaves the upper half of the box empty but for the corner; the merge fills it
        d = (41, 41, 21)
        base = lattice(name, d, 29000, fill=(np.zeros(3), np.array([1.0, 1.0, 0.45])))
        last = cell_centre(d, int(np.prod(d)) - 1) + (_rng(name + "l").random((40, 3)) - 0.5) * 0.2
        upper = _inside(name + "u", 3000, d, fill=(np.array([0.0, 0.0, 0.55]), np.ones(3)))
        return M(name, (), none, base, [(none, _inside(name + "1", 1000, d, fill=(np.zeros(3), np.array([1.0, 1.0, 0.45]))), (None, "build")),
                                        (none, np.concatenate([upper, last]), (None, "merge"))])
    if name == "cross_200000":  # 198 000 + 3 000: the table changes with the set's size, so the kind is rebuilt
        box = (100, 100, 30)
        p = uniform("map", 201000, box)
        p[:2] = [LO, LO + np.array(box)]
        return M(name, (), none, p[:197000], [(none, p[197000:198000], (None, "build")), (none, p[198000:], (None, "build"))])
    if name == "map_second_round":  # MAP_CELLS_LOG2 = 21: more than 256 tiles in index_insert_tile_scan_kernel
        box = (100, 100, 30)
        p = uniform("map", 204001, box)
        p[:2] = [LO, LO + np.array(box)]
        return M(name, (("MAP_CELLS_LOG2", 21),), none, p[:200001], [(none, p[200001:201001], (None, "build")), (none, p[201001:], (None, "merge"))])
    if name == "both_kinds":
        # Both kinds map-sized (25 000 each, 65 536-entry tables). After the first insert has doubled the capacities the shared
        # scratch block still has the builds' size, 64 + 4 (65 536 + 16 + 8) = 262 304 bytes. index_insert_ws_bytes(cells, add) =
        # 16 + 4 (2 (cells + 1) + add + ceil((cells + 1) / 4096)): 3 000 edge points need 16 + 4 (131 074 + 3 000 + 17) = 536 380
        # bytes, so the block is regrown to twice that, 1 072 760. The planar part starts at 536 380 rounded up to 256 = 536 576
        # and needs 16 + 4 (131 074 + 6 000 + 17) = 548 380: 1 084 956 > 1 072 760, the block is regrown again and the edge
        # counts, which were in the old block, are taken once more.
        d = (41, 41, 21)
        return M(name, (), lattice(name + "e", d, 25000), lattice(name + "p", d, 25000),
                 [(_inside(name + "e1", 100, d), _inside(name + "p1", 100, d), ("build", "build")),
                  (_inside(name + "e2", 3000, d), _inside(name + "p2", 6000, d), ("merge", "merge"))])
    raise KeyError(name)


MERGE_SCENES = ("scan_table", "empty_and_last_cells", "cross_200000", "map_second_round", "both_kinds")


def map_table_entries(n, log2=0):
    """the policy of index_build restated for the expectations: above 200 000 points about one entry per two points between
    2^18 and 2^22, or 2^log2 when the option asks for more than the scan-sized table; else 65 536"""
    if n <= 200000:
        return 65536
    if 8 <= log2 <= 24:
        return (1 << log2) if (1 << log2) > 65536 else 65536
    t = 1 << 18
    while t < (1 << 22) and t * 2 < n:
        t <<= 1
    return t
