"""CPU-only: crop_math.h — the rule of the map window (loam_amd/csrc/crop_kernels.hip: the bounds, the skip decision and the
decision per voxel key) — compiled with g++ as a program of its own (tests/hostcheck_crop) against the numpy rule of
tests/crop_common.py, by equality. The GPU tests (test_gpu_crop.py) compare the kernels with the same rule. The last test runs the
same inputs through the program built with AddressSanitizer + UndefinedBehaviorSanitizer."""
import numpy as np
import pytest

import cloudmap_common as CM
import crop_common as X

INF = np.inf
EDGE = X.BIAS - 1  # the largest |cell| a key can hold


def up(x):
    return float(np.nextafter(x, INF))


def dn(x):
    return float(np.nextafter(x, -INF))


def boxes():
    """name -> (centre (3,), lo (3,), hi (3,), leaf)"""
    cases = {}
    for leaf in (0.1, 0.2, 0.5):
        # bounds exactly on a voxel boundary (3 leaf and -2 leaf as the division sees them), one unit in the last place either side
        for name, f in (("on", lambda x: x), ("above", up), ("below", dn)):
            b_hi, b_lo = f(3.0 * leaf), f(-2.0 * leaf)
            cases[f"boundary_{name}_{leaf}"] = ((0.0, 0.0, 0.0), (b_lo, b_lo, b_lo), (b_hi, b_hi, b_hi), leaf)
            cases[f"boundary_{name}_{leaf}_centred"] = ((1.0, -2.0, 0.5), (b_lo, b_lo, b_lo), (b_hi, b_hi, b_hi), leaf)
        cases[f"multiples_{leaf}"] = ((0.0, 0.0, 0.0), (-7 * leaf, 3 * leaf, -leaf), (11 * leaf, 6 * leaf, leaf), leaf)
        cases[f"lo_equals_hi_{leaf}"] = ((0.3, 0.3, 0.3), (0.05, -0.05, 0.0), (0.05, -0.05, 0.0), leaf)
        cases[f"minus_zero_centre_{leaf}"] = ((-0.0, -0.0, -0.0), (-0.0, 0.0, -leaf), (0.0, -0.0, leaf), leaf)
        for a in range(3):
            for side, val in (("lo", -INF), ("hi", INF)):
                lo, hi = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
                (lo if side == "lo" else hi)[a] = val
                cases[f"inf_{side}_{a}_{leaf}"] = ((0.2, 0.2, 0.2), tuple(lo), tuple(hi), leaf)
        cases[f"inf_all_six_{leaf}"] = ((5.0, 5.0, 5.0), (-INF,) * 3, (INF,) * 3, leaf)
        cases[f"inf_inverted_{leaf}"] = ((0.0, 0.0, 0.0), (INF, -1.0, -1.0), (INF, 1.0, 1.0), leaf)  # keeps nothing
        # the sum overflows: defined, keeps or removes everything on that axis
        cases[f"huge_centre_hi_{leaf}"] = ((1e300, 0.0, 0.0), (-1e308, -1.0, -1.0), (1.7e308, 1.0, 1.0), leaf)
        cases[f"huge_centre_both_{leaf}"] = ((1e300, 0.0, 0.0), (1.7e308, -1.0, -1.0), (1.7e308, 1.0, 1.0), leaf)
        cases[f"huge_centre_neg_{leaf}"] = ((0.0, -1e300, 0.0), (-1.0, -1.7e308, -1.0), (1.0, 1e308, 1.0), leaf)
        cases[f"huge_centre_alone_{leaf}"] = ((1e300, 1e300, -1e300), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), leaf)
        for a in range(3):
            for bad in (np.nan, INF, -INF):
                c = [0.5, -0.5, 0.25]
                c[a] = bad
                cases[f"skipped_{a}_{bad}_{leaf}"] = (tuple(c), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), leaf)
        # the cells at +-(2^20 - 1): bounds that reach them, stop one short of them, and lie beyond every key
        far = EDGE * leaf
        cases[f"edge_cells_in_{leaf}"] = ((0.0, 0.0, 0.0), (-far, -far, -far), (up(far), up(far), up(far)), leaf)
        cases[f"edge_cells_out_{leaf}"] = ((0.0, 0.0, 0.0), ((2 - EDGE) * leaf,) * 3, ((EDGE - 2) * leaf,) * 3, leaf)
        cases[f"beyond_every_key_{leaf}"] = ((0.0, 0.0, 0.0), (2.0 * far, -1.0, -1.0), (3.0 * far, 1.0, 1.0), leaf)
    return cases


def probe_cells(flo, fhi):
    """cells around the bounds of every axis, the origin and the cells at +-(2^20 - 1)"""
    per_axis = []
    for a in range(3):
        vals = {0, EDGE, -EDGE, EDGE - 1, 1 - EDGE}
        for b in (flo[a], fhi[a]):
            if np.isfinite(b) and abs(b) < 2 * X.BIAS:
                vals.update(int(b) + d for d in (-1, 0, 1))
        per_axis.append(sorted(v for v in vals if abs(v) <= EDGE))
    cells = [(x, 0, 0) for x in per_axis[0]] + [(0, y, 0) for y in per_axis[1]] + [(0, 0, z) for z in per_axis[2]]
    mid = [int(min(max(0.0 if not np.isfinite(f) else f, -EDGE), EDGE)) for f in flo]
    cells += [(x, mid[1], mid[2]) for x in per_axis[0]] + [(mid[0], y, mid[2]) for y in per_axis[1]] + [(mid[0], mid[1], z) for z in per_axis[2]]
    cells += [(EDGE, EDGE, EDGE), (-EDGE, -EDGE, -EDGE), (EDGE, -EDGE, 0)]
    return cells


def records_of(cases):
    recs, want = [], []
    for name in sorted(cases):
        c, lo, hi, leaf = cases[name]
        pose = np.concatenate([[0.0, 0.0, 0.0, 1.0], c])
        skip, flo, fhi = X.crop_bounds(pose, lo, hi, leaf)
        for cell in probe_cells(flo, fhi):
            key = X.cell_key(cell)
            assert X.key_cell(key) == list(cell)
            recs.append((c, lo, hi, leaf, key))
            want.append((name, cell, skip, flo, fhi, X.keeps(key, flo, fhi)))
    return np.array(recs, dtype=X.CROP_IN), want


def check(program, cases):
    recs, want = records_of(cases)
    got = X.hostcheck_run(program, recs)
    kept = removed = 0
    for g, (name, cell, skip, flo, fhi, keep) in zip(got, want):
        assert int(g["skip"]) == int(skip), (name, cell)
        if skip:
            continue
        assert CM.same_bytes(g["flo"], flo) and CM.same_bytes(g["fhi"], fhi), (name, g["flo"], flo, g["fhi"], fhi)
        assert int(g["keep"]) == int(keep), (name, cell, flo, fhi)
        kept, removed = kept + int(keep), removed + int(not keep)
    return kept, removed


def random_points_in_boxes(n=10000, seed=12):
    """n records: a random box around a random centre at one of the three leaves and the key of a random point inside the closed box"""
    rng = np.random.default_rng(seed)
    recs = np.zeros(n, dtype=X.CROP_IN)
    leaf = rng.choice([0.1, 0.2, 0.5], n)
    c = rng.uniform(-50.0, 50.0, (n, 3))
    lo = -rng.uniform(0.0, 20.0, (n, 3))
    hi = rng.uniform(0.0, 20.0, (n, 3))
    t = rng.uniform(0.0, 1.0, (n, 3))
    t[rng.uniform(size=(n, 3)) < 0.1] = 0.0  # (points on the box's own faces)
    t[rng.uniform(size=(n, 3)) < 0.1] = 1.0
    a, b = c + lo, c + hi  # the corners as the rule forms them
    p = np.clip(a + t * (b - a), a, b)
    ok, v, _ = CM.cells(p, leaf[:, None])
    assert ok.all()
    recs["c"], recs["lo"], recs["hi"], recs["leaf"], recs["key"] = c, lo, hi, leaf, CM.pack(v)
    return recs


@pytest.fixture(scope="module")
def program():
    return X.hostcheck_program()


def test_bounds_skip_and_keys_equal_the_numpy_rule(program):
    kept, removed = check(program, boxes())
    assert kept > 500 and removed > 500  # (both decisions are taken often)


def test_what_the_named_boxes_are_there_for():
    """asserted on the numpy rule alone"""
    b = boxes()
    _, flo, fhi = X.crop_bounds(np.concatenate([[0, 0, 0, 1.0], b["boundary_on_0.1"][0]]), *b["boundary_on_0.1"][1:])
    assert fhi[0] in (2.0, 3.0) and flo[0] in (-2.0, -3.0)  # 0.1 is not representable: where the boundary lands is the division's business
    for leaf in (0.2, 0.5):
        c, lo, hi, _ = b[f"boundary_on_{leaf}"]
        on = X.crop_bounds(None, lo, hi, leaf)
        below = X.crop_bounds(None, *b[f"boundary_below_{leaf}"][1:])
        assert on[2][0] - below[2][0] in (0.0, 1.0) and on[2][0] >= 2.0
    skip, flo, fhi = X.crop_bounds(None, *b["inf_all_six_0.2"][1:])
    assert not skip and (flo == -INF).all() and (fhi == INF).all()
    skip, flo, fhi = X.crop_bounds(np.concatenate([[0, 0, 0, 1.0], b["huge_centre_hi_0.2"][0]]), *b["huge_centre_hi_0.2"][1:])
    assert not skip and fhi[0] == INF and flo[0] == -INF and X.keeps(X.cell_key((EDGE, 0, 0)), flo, fhi)
    skip, flo, fhi = X.crop_bounds(np.concatenate([[0, 0, 0, 1.0], b["huge_centre_both_0.2"][0]]), *b["huge_centre_both_0.2"][1:])
    assert not skip and flo[0] == INF and fhi[0] == INF and not X.keeps(X.cell_key((0, 0, 0)), flo, fhi)
    skip, flo, fhi = X.crop_bounds(np.concatenate([[0, 0, 0, 1.0], b["huge_centre_alone_0.2"][0]]), *b["huge_centre_alone_0.2"][1:])
    assert not skip and not X.keeps(X.cell_key((EDGE, EDGE, -EDGE)), flo, fhi)
    for a in range(3):
        for bad in (np.nan, INF, -INF):
            c, lo, hi, leaf = b[f"skipped_{a}_{bad}_0.5"]
            assert X.crop_bounds(np.concatenate([[0, 0, 0, 1.0], c]), lo, hi, leaf)[0]
    _, flo, fhi = X.crop_bounds(None, *b["edge_cells_in_0.5"][1:])
    assert X.keeps(X.cell_key((EDGE, EDGE, EDGE)), flo, fhi) and X.keeps(X.cell_key((-EDGE, -EDGE, -EDGE)), flo, fhi)
    _, flo, fhi = X.crop_bounds(None, *b["edge_cells_out_0.5"][1:])
    assert not X.keeps(X.cell_key((EDGE, 0, 0)), flo, fhi) and X.keeps(X.cell_key((EDGE - 2, 0, 0)), flo, fhi)
    # -0.0 and +0.0 centres give the same decisions
    c, lo, hi, leaf = b["minus_zero_centre_0.2"]
    a0, b0 = X.crop_bounds(np.array([0, 0, 0, 1.0, -0.0, -0.0, -0.0]), lo, hi, leaf)[1:], X.crop_bounds(None, lo, hi, leaf)[1:]
    assert (a0[0] == b0[0]).all() and (a0[1] == b0[1]).all()


def test_every_point_of_the_closed_box_lies_in_a_kept_cell(program):
    """the property the header states: 10 000 random points inside random boxes, faces included"""
    recs = random_points_in_boxes()
    got = X.hostcheck_run(program, recs)
    assert not got["skip"].any()
    assert got["keep"].all(), int((got["keep"] == 0).sum())
    for r in recs[:200]:  # ... and the numpy rule says the same
        _, flo, fhi = X.crop_bounds(np.concatenate([[0, 0, 0, 1.0], r["c"]]), r["lo"], r["hi"], float(r["leaf"]))
        assert X.keeps(int(r["key"]), flo, fhi)


def test_folding_the_centre_on_the_host_gives_the_same_bounds(program):
    """0.0 + x == x: the centre added to lo and hi by the caller, and no pose"""
    rng = np.random.default_rng(3)
    recs = random_points_in_boxes(500, seed=4)
    folded = recs.copy()
    folded["lo"], folded["hi"], folded["c"] = recs["c"] + recs["lo"], recs["c"] + recs["hi"], 0.0
    folded["key"] = recs["key"] = X.cell_key((int(rng.integers(-50, 50)), 3, -3))
    a, b = X.hostcheck_run(program, recs), X.hostcheck_run(program, folded)
    assert CM.same_bytes(a, b)


def test_the_sanitized_program_agrees():
    program = X.hostcheck_program(san=True)
    check(program, boxes())
    assert X.hostcheck_run(program, random_points_in_boxes(2000))["keep"].all()
