"""CPU-only: the exact search of one late query by a row of 16 lanes (reg_math.h: knn_exact_block_row16, what
associate_fit_late_kernel runs) in its host form — a plain loop over 16 virtual lanes where the device takes a DPP row minimum —
against the one-lane search it replaces (knn_search). tests/hostcheck_late_rows is a stand-alone program compiled with g++; it
prints one line per case and the same program runs under AddressSanitizer + UndefinedBehaviorSanitizer.

Per query: where the row decides, kept, the k slots of the KnnResult (distances bit for bit, positions, original indices), worst
and count must be knn_search's; where it does not, it must have one of its three reasons (`far`: the query's cell is more than
one cell off the grid; `guard`: the block's k best do not pass knn_done's test, which the program repeats on a one-lane walk of
the block; `cap`: more than 256 candidates) and report no list. Cases: random sets at ~50 points per cubic metre and a 0.5 m cell
(160 - 190 candidates a block) with k = 1 .. 5, with and without a radius, queries all over the box, in the corner cells and up to
three cells outside the grid; a sparse set (the guard); radii that keep 0 .. 5 of the five nearest; a three-point set; a
coplanar set (nz = 1); the 9 x 9 x 8 lattice at 0.125 m with queries on lattice points, edge midpoints and face centres (exact
ties that only the original index orders; the storage order inside the cells is shuffled); every point three times over; 252 and
300 points in one cell (the row's capacity); and the selection step alone on candidates with six distinct distances dealt to
the lanes at random, against one list that saw them all."""
import os
import subprocess

import pytest

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck_late_rows")
FIELDS = ("queries", "decided", "far", "guard", "cap", "mismatches", "short_lists", "max_block")
CASES = {"random_a", "corners_a", "random_b", "corners_b", "sparse", "radius", "three_points", "flat", "lattice", "duplicates",
         "crowded_252", "crowded_300", "deal"}


def run(target, binary):
    subprocess.check_call(["make", "-s", "-C", DIR] + ([target] if target else []))
    p = subprocess.run([os.path.join(DIR, binary)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    rows = {}
    for line in p.stdout.splitlines():
        name, *nums = line.split()
        rows[name] = dict(zip(FIELDS, map(int, nums)))
    return p, rows


@pytest.fixture(scope="module")
def rows():
    p, rows = run(None, "hostcheck_late_rows")
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    return rows


def test_every_case_ran(rows):
    assert set(rows) == CASES
    assert all(r["queries"] >= 200 for r in rows.values())
    assert sum(r["decided"] for n, r in rows.items() if n != "deal") >= 5000  # a few thousand blocks decided by the row
    assert all(r["decided"] + r["far"] + r["guard"] + r["cap"] == r["queries"] for r in rows.values())


def test_the_row_equals_the_one_lane_search_on_every_query(rows):
    for name, r in rows.items():
        assert r["mismatches"] == 0, (name, r)


def test_dense_sets_are_decided_by_the_row(rows):
    for name in ("random_a", "random_b", "flat", "duplicates", "lattice", "radius", "three_points"):
        r = rows[name]
        assert r["decided"] > 0.95 * r["queries"] and r["far"] == 0, (name, r)
    assert rows["lattice"]["decided"] == rows["lattice"]["queries"]  # (no face of a block inside the grid is nearer than the ties)
    assert rows["random_b"]["max_block"] > 128  # more than one batch of 16 x 8 candidates


def test_every_way_out_is_reached(rows):
    assert rows["sparse"]["guard"] > 1000 and rows["sparse"]["short_lists"] > 100  # the block does not prove the list; fewer than k in range
    assert rows["corners_a"]["far"] + rows["corners_a"]["cap"] + rows["corners_a"]["guard"] > 0
    assert rows["corners_a"]["decided"] > 1000 and rows["corners_b"]["decided"] > 1000  # (corner cells, one cell outside; beyond, out of range: kept 0)
    assert rows["radius"]["short_lists"] > 1000  # kept = 0 .. 4 under the radius
    assert rows["three_points"]["short_lists"] > 50  # fewer points than k
    assert rows["deal"]["short_lists"] > 100


def test_the_capacity_is_256_candidates(rows):
    a, b = rows["crowded_252"], rows["crowded_300"]
    assert a["decided"] == a["queries"] and a["max_block"] == 252
    assert b["cap"] == b["queries"] and b["decided"] == 0


def test_the_program_is_clean_under_asan_and_ubsan():
    p, rows = run("san", "hostcheck_late_rows_san")
    assert p.returncode == 0, p.stdout + p.stderr
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr
    assert set(rows) == CASES
