"""CPU-only: the plane k-NN's round 1 as two halves (reg_math.h: knn_lean_round1 in its unverified form — the search-over
threshold taken in front of the walk, positions and a count word from the FP32 keys alone — then knn_handoff_verify on the
gathered FP64 points, which is what the plane fit kernel runs) against the one function of before (knn_lean_round1 ->
knn_lean_finish) and against a brute-force exact k-NN. tests/hostcheck_handoff is a stand-alone program compiled with g++; it
prints one line per case and the same program runs under AddressSanitizer + UndefinedBehaviorSanitizer.

Per query, undecided-or-not, kept and every position must be equal between the two forms (`mismatches`), and a decided query
must hold the brute-force answer (`brute_mismatches`). Cases: random sets of 600 points (2 m box) and 5 000 points (4 m box)
at a 0.5 m cell, queries all over the box, in the corner cells and up to three cells outside the grid, with and without a
radius; a sparse set and radii below the neighbours' distances (fewer than five points in range); a three-point set; the
9 x 9 x 8 lattice at 0.1 m with queries on lattice points, edge midpoints (exact ties) and a millimetre off lattice points.
(600 points in the 4 m box have the fifth neighbour as far away as the block's faces: 28 % undecided in either form; the 2 m
box gives them the density of the larger set.)"""
import os
import subprocess

import pytest

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck_handoff")
FIELDS = ("queries", "undecided_old", "undecided_new", "refused", "mismatches", "brute_mismatches", "short_lists")


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
    p, rows = run(None, "hostcheck_handoff")
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    return rows


def test_every_case_ran(rows):
    assert set(rows) == {"random_a", "corners_a", "random_b", "corners_b", "sparse", "three_points", "lattice"}
    assert all(r["queries"] >= 200 for r in rows.values())


def test_both_forms_agree_on_every_query_and_with_brute_force(rows):
    for name, r in rows.items():
        assert r["mismatches"] == 0 and r["brute_mismatches"] == 0, (name, r)
        assert r["undecided_old"] == r["undecided_new"], (name, r)


def test_random_sets_are_decided_and_the_lattice_is_not(rows):
    for name in ("random_a", "random_b"):
        assert rows[name]["undecided_old"] < 0.01 * rows[name]["queries"], (name, rows[name])
    lat = rows["lattice"]
    assert lat["undecided_old"] > 0.5 * lat["queries"], lat
    # on the lattice the keys alone select (no face of the block lies inside the grid): what is undecided is refused by the
    # checks on the gathered points; and some of the jittered queries ARE decided there, by both forms alike
    assert lat["refused"] > 0.5 * lat["queries"] and lat["undecided_new"] < lat["queries"], lat


def test_the_other_exits_are_reached(rows):
    assert rows["sparse"]["short_lists"] > 100       # decided with fewer than five neighbours within the radius
    assert rows["sparse"]["undecided_old"] > 100     # the block's faces closer than the fifth neighbour: queued
    assert rows["corners_a"]["undecided_old"] > 0 and rows["corners_b"]["undecided_old"] > 0  # (beyond one cell outside the grid)
    assert rows["three_points"]["undecided_old"] == 0


def test_the_program_is_clean_under_asan_and_ubsan():
    p, rows = run("san", "hostcheck_handoff_san")
    assert p.returncode == 0, p.stdout + p.stderr
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr
    assert len(rows) == 7
