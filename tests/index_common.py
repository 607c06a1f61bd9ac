"""The structure of a target index, checked in plain numpy against the points it was built from: no code shared
with the kernels or with the hostcheck. A census is a capi.IndexCensus (loamx_target_index_census) or a dict with the same
fields (hostcheck_lib.build_grid: the CPU leg, tests/test_index_hostcheck.py)."""
import numpy as np

REL_PAD = np.float32(3.0e38)  # kRelPad (reg_math.h)
LDS_CELLS = 32768             # kGridLdsCells: cells per pass of the single-workgroup builds
SCAN_TILE = 4096              # kScanTile: table entries per tile of the gridbig_* / index_insert_* scans
TILES_PER_ROUND = 256         # kScanThreads: tiles per round of the tile-sum scans


def field(c, name):
    return c[name] if isinstance(c, dict) else getattr(c, name)


def ncell_of(c):
    d = field(c, "dims")
    return int(d[0]) * int(d[1]) * int(d[2])


def cells_of(c, xyz):
    """grid_cell_of_point restated: clip(floor((p - o) * inv_h), 0, dim - 1) per axis, x fastest — three float64 operations, exact"""
    o, inv_h, d = np.asarray(field(c, "origin"), dtype=np.float64), np.float64(field(c, "inv_h")), field(c, "dims")
    ijk = []
    for a in range(3):
        v = np.floor((xyz[:, a] - o[a]) * inv_h)
        ijk.append(np.clip(v, 0, d[a] - 1).astype(np.int64))
    return (ijk[2] * int(d[1]) + ijk[1]) * int(d[0]) + ijk[0]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def check_index(c, pts):
    """Raises AssertionError unless census `c` describes a correct index of `pts` (in insertion order)."""
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    n = len(pts)
    xyz, orig, rel = field(c, "xyz"), field(c, "orig"), field(c, "rel")
    assert field(c, "n") == n and field(c, "n_points") == n, (field(c, "n"), field(c, "n_points"), n)
    assert xyz.shape == (n, 3) and orig.shape == (n,) and rel.shape == (3, n + 4)
    # 1. permutation
    assert np.array_equal(np.sort(orig.astype(np.int64)), np.arange(n)), "orig is not a permutation of 0 .. n - 1"
    assert np.array_equal(bits(xyz), bits(pts[orig.astype(np.int64)])), "a sorted point is not the point its orig names"
    # 2. cells
    ncell = ncell_of(c)
    assert ncell >= 1 and min(field(c, "dims")) >= 1
    if field(c, "table_valid"):
        cs = field(c, "cell_start").astype(np.int64)
        assert cs.shape == (ncell + 1,)
        cell = cells_of(c, xyz)
        assert n == 0 or (np.diff(cell) >= 0).all(), "the sorted points are not in cell order"
        assert cs[0] == 0 and cs[ncell] == n, (cs[0], cs[ncell], n)
        assert (np.diff(cs) >= 0).all(), "the cell table is not monotone"
        pop = np.bincount(cell, minlength=ncell)
        bad = np.nonzero(np.diff(cs) != pop)[0]
        assert len(bad) == 0, ("cell populations differ from the table", bad[:5], np.diff(cs)[bad[:5]], pop[bad[:5]])
    # 3. float copies and their pads
    o = np.asarray(field(c, "origin"), dtype=np.float64)
    for a in range(3):
        want = (xyz[:, a] - o[a]).astype(np.float32)
        assert np.array_equal(bits(rel[a, :n]), bits(want)), ("rel plane differs from float32(xyz - origin)", a)
        assert np.array_equal(bits(rel[a, n:]), bits(np.full(4, REL_PAD))), ("pad entries behind rel plane", a, rel[a, n:])


def check_grid_choice(c, pts, radius, cells_cap, Hc):
    """4. (full builds) origin = the exact box minimum; h, inv_h and the dimensions = the g++ build of grid_choose over the exact
    bounding box, h bit for bit (Hc: hostcheck_lib)"""
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    h, dims = Hc.grid_choose_cap(pts, radius, cells_cap)
    assert tuple(field(c, "dims")) == dims, (field(c, "dims"), dims)
    assert bits(np.float64(field(c, "h")).reshape(1))[0] == bits(np.float64(h).reshape(1))[0], (field(c, "h"), h)
    assert bits(np.float64(field(c, "inv_h")).reshape(1))[0] == bits((np.float64(1.0) / np.float64(h)).reshape(1))[0]
    want_o = pts.min(axis=0) if len(pts) else np.zeros(3)
    assert np.array_equal(bits(np.asarray(field(c, "origin"), dtype=np.float64)), bits(want_o)), (field(c, "origin"), want_o)
    assert ncell_of(c) <= cells_cap


def check_desc_kept(before, after):
    """after a merge: the grid of the last full build, with the point count updated"""
    for f in ("h", "inv_h"):
        assert bits(np.float64(field(before, f)).reshape(1))[0] == bits(np.float64(field(after, f)).reshape(1))[0], f
    assert tuple(field(before, "dims")) == tuple(field(after, "dims"))
    assert np.array_equal(bits(np.asarray(field(before, "origin"), dtype=np.float64)), bits(np.asarray(field(after, "origin"), dtype=np.float64)))
    assert field(after, "n_points") == field(after, "n")


def recount(c, pts):
    """the cell table a census's grid implies for `pts`, by numpy alone"""
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    pop = np.bincount(cells_of(c, pts), minlength=ncell_of(c))
    return np.concatenate([[0], np.cumsum(pop)]).astype(np.uint32)


def ceil_div(a, b):
    return -(-a // b)


# ---- mutations of a correct structure (the CPU leg requires check_index to refuse each) -----------------------------
def _copy(c):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}


def mutate(c, how):
    """a dict census with ONE defect; the census must hold at least two occupied cells"""
    m = _copy(c)
    cs, n = m["cell_start"].astype(np.int64), m["n"]
    occ = np.nonzero(np.diff(cs) > 0)[0]
    a, b = int(cs[occ[0]]), int(cs[occ[1]])  # first positions of the first two occupied cells
    if how == "moved_point":  # a point of the second occupied cell filed in the first one's range
        for arr in (m["xyz"], m["orig"]):
            arr[[a, b]] = arr[[b, a]]
        m["rel"][:, [a, b]] = m["rel"][:, [b, a]]
    elif how == "table_entry":
        m["cell_start"][occ[1]] += 1
    elif how == "rel_ulp":
        bits(m["rel"])[1, n // 2] ^= 1
    elif how == "pad":
        m["rel"][2, n + 3] = np.float32(0.0)
    elif how == "orig_swap":
        m["orig"][[a, b]] = m["orig"][[b, a]]
    else:
        raise KeyError(how)
    return m


MUTATIONS = ("moved_point", "table_entry", "rel_ulp", "pad", "orig_swap")
