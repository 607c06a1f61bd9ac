"""CPU-only: distance_math.h — the rule of the occupancy distance field (loam_amd/csrc/distance_kernels.hip: the x-pass on mask
words, the y- and z-pass in both early-exit forms, the metres) — compiled with g++ as a program of its own
(tests/hostcheck_distance) against the brute-force numpy model of tests/distance_common.py, by equality of d2, offsets and metres.
The model itself is checked against scipy's exact Euclidean transform. The GPU tests (test_gpu_distance.py) compare the kernels
with the same model on the same named cases. The last test runs the cases through the program built with AddressSanitizer +
UndefinedBehaviorSanitizer, as a child process."""
import numpy as np
import pytest

import distance_common as D

CASES = D.named_cases()
LEAF = 0.2


@pytest.fixture(scope="module")
def program():
    return D.hostcheck_program()


@pytest.fixture(scope="module")
def random_boxes():
    boxes = D.random_boxes()
    return boxes, [D.case_field(b, LEAF) for b in boxes]


def assert_fields_equal(got, want, what):
    for name, g, w in zip(("d2", "offset", "metres"), got, want):
        assert g.shape == w.shape and D.same_bytes(g, w), (what, name, g, w)


def check(program, cases, wants, names):
    for early in (1, 0):
        for name, got, want in zip(names, D.hostcheck_run(program, cases, early, LEAF), wants):
            assert_fields_equal(got, want, (name, "early" if early else "whole window"))


def test_the_named_cases_equal_the_model_in_both_forms(program):
    names = sorted(CASES)
    cases = [CASES[n] for n in names]
    check(program, cases, [D.case_field(c, LEAF) for c in cases], names)


def test_what_the_named_cases_are_there_for():
    """asserted on the model alone"""
    f = lambda name: D.case_field(CASES[name], LEAF)
    d2, off, m = f("cap_25_reported")
    assert d2.item() == 25 and off.reshape(-1).tolist() == [3, 4, 0] and m.item() == np.float32(np.sqrt(25.0) * LEAF)
    d2, off, m = f("cap_26_far")
    assert d2.item() == D.FAR and not off.any() and np.isposinf(m.item())
    d2, off, _ = f("cap_65025_reported")
    assert d2.reshape(-1).tolist() == [65025, 64666] and off.reshape(2, 3).tolist() == [[180, 180, 15], [179, 180, 15]]
    assert f("cap_65026_far")[0].reshape(-1).tolist() == [D.FAR, 64802]  # (voxel 0: 65161 is beyond the cap; voxel 1 is one nearer)
    for a in range(3):
        assert f(f"cap_axis_{a}_plus_255")[0].reshape(-1)[0] == 65025 and f(f"cap_axis_{a}_plus_256")[0].reshape(-1)[0] == D.FAR
        assert f(f"cap_axis_{a}_minus_255")[0].reshape(-1)[0] == 65025 and (f(f"cap_axis_{a}_minus_256")[0] == D.FAR).all()
    # ties: the lowest z, then the lowest y, then the lowest x
    for d in (1, 3):
        centre = lambda name: f(name)[1][2, 2, 2].tolist()
        assert centre(f"ties_pm{d}_axes_0") == [-d, 0, 0] and centre(f"ties_pm{d}_axes_1") == [0, -d, 0] and centre(f"ties_pm{d}_axes_2") == [0, 0, -d]
        assert centre(f"ties_pm{d}_axes_01") == [0, -d, 0] and centre(f"ties_pm{d}_axes_02") == [0, 0, -d] and centre(f"ties_pm{d}_axes_012") == [0, 0, -d]
        assert centre(f"ties_cube_corners_{d}") == [-d, -d, -d] and f(f"ties_cube_corners_{d}")[0][2, 2, 2] == 3 * d * d
    assert f("stop_edge_lower_y")[1].reshape(-1).tolist() == [0, -2, 0] and f("stop_edge_higher_y")[1].reshape(-1).tolist() == [-2, 0, 0]
    assert f("stop_edge_lower_z")[1].reshape(-1).tolist() == [0, 0, -2] and f("stop_edge_higher_z")[1].reshape(-1).tolist() == [0, -2, 0]
    assert f("stop_edge_3_4_5")[1].reshape(-1).tolist() == [0, 0, -5] and f("stop_edge_3_4_5")[0].item() == 25
    # the halo: an obstacle R outside the box is seen by the nearest face, one at R + 1 by nobody
    for a in range(3):
        for tag in ("above", "below"):
            seen, unseen = f(f"halo_axis_{a}_{tag}_R")[0], f(f"halo_axis_{a}_{tag}_R_plus_1")[0]
            assert (seen == 9).sum() == 1 and (seen != D.FAR).sum() == 1 and (unseen == D.FAR).all()
    d2, off, _ = f("last_bit_then_first_bit")  # voxel x = 60 stands at position 64, the obstacle x = 59 at position 63
    assert d2[0, 0, 60 - 56] == 1 and off[0, 0, 60 - 56].tolist() == [-1, 0, 0] and d2[0, 1, 124 - 56] == 1
    assert (f("window_of_three_words")[0] != D.FAR).all() and (f("window_of_three_words_far")[0] == D.FAR).any()
    d2, _, m = f("no_obstacles")
    assert (d2 == D.FAR).all() and np.isposinf(m).all()
    assert f("slice_ties")[1][2, 2].tolist() == [0, -2] and f("slice_cap")[0].reshape(-1).tolist() == [25, 20]


def test_random_boxes_equal_the_model_in_both_forms(program, random_boxes):
    boxes, wants = random_boxes
    assert len(boxes) == 200 and {b["R"] for b in boxes} == set(range(1, 8))
    check(program, boxes, wants, list(range(len(boxes))))
    seen = np.concatenate([w[0].ravel() for w in wants])
    assert (seen == 0).any() and (seen == D.FAR).any() and ((seen > 0) & (seen < D.FAR)).sum() > 1000


def test_the_model_equals_scipys_exact_transform_wherever_the_cap_allows(random_boxes):
    boxes, wants = random_boxes
    compared = 0
    for b, (d2, _, _) in zip(boxes, wants):
        A = 2 if b["slice"] else 3
        e2 = D.edt_d2(b["obst"][:, :A], b["vmin"], b["dims"], b["R"])
        near = e2 <= b["R"] ** 2
        assert (d2[near] == e2[near]).all() and (d2[~near] == D.FAR).all()
        compared += int(near.sum())
    assert compared > 5000


def test_metres_round_each_operation_on_its_own(program):
    """every d2 up to the cap at a leaf that is not representable: one field whose squared distances run through 0 .. 255^2"""
    case = dict(obst=np.array([[-1, 0, 0]]), vmin=np.array([0, 0, 0]), dims=np.array([255, 1, 1]), R=255)
    want = D.case_field(case, 0.1)
    assert want[0].reshape(-1).tolist() == [(x + 1) ** 2 for x in range(255)]
    got = D.hostcheck_run(program, [case], 1, 0.1)[0]
    assert_fields_equal(got, want, "metres")


def test_the_sanitized_program_agrees(random_boxes):
    program = D.hostcheck_program(san=True)
    names = sorted(CASES)
    cases = [CASES[n] for n in names]
    check(program, cases, [D.case_field(c, LEAF) for c in cases], names)
    boxes, wants = random_boxes
    check(program, boxes[:60], wants[:60], list(range(60)))
