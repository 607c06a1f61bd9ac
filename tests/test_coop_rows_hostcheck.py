"""CPU-only: the cooperative search of one listed query by a row of L lanes (reg_math.h: knn_coop_search_rows, what
associate_knn_coop_kernel runs) in its host form — plain loops over L virtual lanes where the device takes a ballot, a lane read
and a DPP row minimum — against the one-lane searches on the same grid, table and points. tests/hostcheck_coop_rows is a
stand-alone program compiled with g++; it reads the cases this test writes, prints one line per case and L = 16, 32, 64, and the
same program runs under AddressSanitizer + UndefinedBehaviorSanitizer.

Per query: the return code and all KM position slots must be knn_search_keyed's (kept >= 0, or -1 undecided); where the keys
decide, count and positions must be knn_search's (the exact collector) as well; -2 (not applicable: the caller runs the one-lane
search) is counted. Cases, from tests/assoc_scenes.py where it has them: `sparse` at k = 3, 5, 8, 16 (isolated queries of a
30 m cube, most with fewer than k points in range), `sparse_few`, `outside` (queries 0 .. 5 and 9 cells off the grid), a
300-point set with queries 1.0 - 1.9 m from their nearest point (h = 0.5: shells 3 - 5 are walked) at k = 5 and 16 (fewer than k
inside the radius), the lattice (exact ties: every query must come back -1) and the rod (more than 64 shells: every query -2);
then k + 1 draws from keys dealt to the lanes at random against the sorted list, 4 000 deals per (KM, L); and the kernel's deal
of a pair's listed entries to workgroups, rows and turns (its loop, stepped by the kernel's own knn_coop_deal_first / _step), 4 000
random lists with random reason bits per row width: every entry taken exactly once, plain ones by row t mod (rows x workgroups) in
turn t / (rows x workgroups), wide and tied ones by the wavefront of the workgroup whose turn holds them."""
import os
import subprocess

import numpy as np
import pytest

import assoc_scenes as S

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck_coop_rows")
FIELDS = ("k", "queries", "decided", "undecided", "na", "mismatches", "short_lists", "max_shells")
LANES = (16, 32, 64)


def isolated(k):
    """300 uniform points in an 8 m cube (h = r / 4 = 0.5: 16^3 = 4096 cells <= 16 n) and the queries, of 6 000 drawn in and around the
    cube, whose nearest point is 1.0 - 1.9 m away: no block of 3x3x3 or 5x5x5 cells proves their list; the radius closes at shell 5"""
    rng = np.random.default_rng(120)
    tgt = rng.uniform(0.0, 8.0, (300, 3))
    cand = rng.uniform(-1.0, 9.0, (6000, 3))
    nearest = np.sqrt(((cand[:, None, :] - tgt[None, :, :]) ** 2).sum(-1)).min(axis=1)
    return S.scene("isolated_k%d" % k, "plane", S.NONE, cand[(nearest >= 1.0) & (nearest <= 1.9)][:800], S.NONE, tgt, k_p=k)


def cases():
    out = [(S.sparse(k)._replace(name="sparse_k%d" % k), 0) for k in (3, 5, 8, 16)]
    out += [(S.sparse_few(), 0), (S.outside(), 0), (isolated(5), 0), (isolated(16), 0), (S.lattice(5), -1), (S.rod(), -2)]
    return out


def write_case(path, s, expect):
    q, t, k, r = S.sets(s)
    with open(path, "wb") as f:
        np.array([len(t), len(q), k, expect], dtype=np.int32).tofile(f)
        np.array([r], dtype=np.float64).tofile(f)
        np.ascontiguousarray(t, dtype=np.float64).tofile(f)
        np.ascontiguousarray(q, dtype=np.float64).tofile(f)


@pytest.fixture(scope="module")
def case_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("coop_rows")
    files = []
    for s, expect in cases():
        files.append(str(d / (s.name + ".bin")))
        write_case(files[-1], s, expect)
    return files


def run(target, binary, files):
    subprocess.check_call(["make", "-s", "-C", DIR] + ([target] if target else []))
    p = subprocess.run([os.path.join(DIR, binary)] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    rows = {}
    for line in p.stdout.splitlines():
        name, lanes, *nums = line.split()
        rows[(name, int(lanes)) if name != "deal" else (name, int(lanes), int(nums[0]))] = dict(zip(FIELDS, map(int, nums)))
    return p, rows


@pytest.fixture(scope="module")
def rows(case_files):
    p, rows = run(None, "hostcheck_coop_rows", case_files)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    return rows


NAMES = ("sparse_k3", "sparse_k5", "sparse_k8", "sparse_k16", "sparse_few", "outside", "isolated_k5", "isolated_k16", "lattice_k5", "rod")
DEALS = {("deal", 16, 5), ("deal", 32, 5), ("deal", 16, 8), ("deal", 32, 16)}
ENTRY_DEALS = {("entries", 4), ("entries", 2)}


def test_every_case_ran_at_every_row_width(rows):
    assert set(rows) == {(n, lanes) for n in NAMES for lanes in LANES} | DEALS | ENTRY_DEALS
    for key, r in rows.items():
        assert r["queries"] > 0 and r["decided"] + r["undecided"] + r["na"] == r["queries"], (key, r)
    assert all(rows[d]["queries"] == 4000 and rows[d]["short_lists"] > 100 for d in DEALS)
    # the deal of list entries to workgroups, rows and turns: 4 000 lists each, more than a thousand with a second turn, up to ten turns
    assert all(rows[d]["queries"] == 4000 and rows[d]["short_lists"] > 1000 and rows[d]["max_shells"] >= 10 for d in ENTRY_DEALS)
    for n, k in (("sparse_k3", 3), ("sparse_k5", 5), ("sparse_k8", 8), ("sparse_k16", 16), ("isolated_k16", 16)):
        assert all(rows[(n, lanes)]["k"] == k for lanes in LANES)


def test_the_rows_equal_the_one_lane_searches_on_every_query(rows):
    for key, r in rows.items():
        assert r["mismatches"] == 0, (key, r)


def test_the_scenes_reach_what_they_are_for(rows):
    for lanes in LANES:
        for n in ("sparse_k3", "sparse_k5", "sparse_k8", "sparse_k16", "sparse_few", "isolated_k5", "isolated_k16"):
            r = rows[(n, lanes)]
            assert r["decided"] == r["queries"], (n, lanes, r)
        assert rows[("sparse_k5", lanes)]["short_lists"] > 100 and rows[("isolated_k16", lanes)]["short_lists"] > 0  # fewer than k inside the radius
        assert rows[("isolated_k5", lanes)]["queries"] >= 100 and rows[("isolated_k5", lanes)]["max_shells"] >= 5  # shells 3 - 5
        assert rows[("sparse_k5", lanes)]["max_shells"] >= 4
        o = rows[("outside", lanes)]
        assert o["decided"] == o["queries"] and o["max_shells"] >= 6 + 5  # (h = 0.49: ceil(r / h) + 1 = 6 shells, + out = 5)
        t, rod = rows[("lattice_k5", lanes)], rows[("rod", lanes)]
        assert t["undecided"] == t["queries"] == 300  # exact ties: -1
        assert rod["na"] == rod["queries"] == 200     # more than 64 shells: -2


def test_the_program_is_clean_under_asan_and_ubsan(case_files):
    p, rows = run("san", "hostcheck_coop_rows_san", case_files)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr
    assert set(rows) == {(n, lanes) for n in NAMES for lanes in LANES} | DEALS | ENTRY_DEALS
