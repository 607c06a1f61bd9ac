"""CPU-only: surfel_math.h — the per-point terms and surfel_finish of the surfel map kernels (loam_amd/csrc/surfel_kernels.hip)
— compiled with g++ as a program of its own (tests/hostcheck_surfel) against the Python model of tests/surfel_common.py, by
equality, voxel by voxel. The GPU tests (test_gpu_surfel.py) compare the kernels with the same model. The last test runs the
same inputs through the program built with AddressSanitizer + UndefinedBehaviorSanitizer."""
import numpy as np
import pytest

import cloudmap_common as CM
import surfel_common as M

CASES = M.shared_cases()


def model_of(leaf, pts, pose, min_range=0.0, max_range=120.0):
    m = M.SurfelMapModel(leaf, min_range, max_range)
    m.add(pts, poses=None if pose is None else np.asarray(pose)[None])
    return m


def check_points(program, leaf, pts, pose, min_range=0.0, max_range=120.0):
    got = M.hostcheck_points(program, pts, pose, leaf, min_range, max_range)
    what, v, key, q, w = M.point_terms(np.asarray(pts, dtype=np.float64), pose, leaf, min_range, max_range)
    assert np.array_equal(got["what"].astype(np.int64), what)
    used = what == CM.USED
    assert np.array_equal(got["key"][used], key[used])
    want = np.concatenate([q, np.stack([q[:, a] * q[:, b] for a, b in M.PAIRS], axis=1), w.view(np.uint64)], axis=1)
    assert np.array_equal(got["m"][used], want[used])
    assert not got["m"][~used].any()  # a point without a voxel carries zeros in all twelve
    return int(used.sum())


def check_finish(program, entries, leaf, what=""):
    got = M.hostcheck_finish(program, entries, leaf)
    want = M.records([M.finish(e[0], e[1], e[2], e[3], e[4], e[5], leaf) for e in entries])
    M.assert_records_equal(got, want, what)
    return got


@pytest.fixture(scope="module")
def program():
    return M.hostcheck_program()


@pytest.mark.parametrize("name", sorted(CASES))
def test_shared_case_points_and_records_equal_the_model(program, name):
    leaf, pts, pose = CASES[name]
    assert check_points(program, leaf, pts, pose) > 0
    m = model_of(leaf, pts, pose)
    assert m.vox and m.used > 0, name
    got = check_finish(program, list(m.vox.values()), leaf, name)
    for r in got:
        assert abs(float(np.dot(r["normal"], r["normal"])) - 1.0) < 1e-12 and r["count"] >= 1
        assert r["eval"][0] <= r["eval"][1] <= r["eval"][2]


def test_what_the_named_cases_are_there_for():
    """each named case reaches the path its name promises (asserted on the model alone)"""
    rec = {name: model_of(*CASES[name]).emit()[0] for name in CASES}
    assert all(len(rec[n]) == 1 for n in ("one_point", "two_points", "three_points"))
    one = rec["one_point"][0]
    assert not one["cov"].any() and not one["eval"].any() and one["normal"].tolist() == [-1.0, -0.0, -0.0]  # three equal eigenvalues: column 0; no pose: seen from the origin
    # ties keep column order: (0, s, s) -> x, y, z normal for the three planes; the cube's three equal eigenvalues -> column 0
    for name, axis in (("coplanar_yz", 0), ("coplanar_zx", 1), ("coplanar_xy", 2)):
        r = rec[name][0]
        assert r["eval"][0] == 0.0 and r["eval"][1] == r["eval"][2] > 0.0 and abs(r["normal"][axis]) == 1.0, name
    cube = rec["cube_equal_eigenvalues"][0]
    assert cube["eval"][0] == cube["eval"][1] == cube["eval"][2] > 0.0 and abs(cube["normal"][0]) == 1.0
    for name in CASES:
        if name.startswith("diagonal_"):
            r, order = rec[name][0], [int(c) for c in name[-3:]]
            assert not r["cov"][[1, 2, 4]].any() and abs(r["normal"][order.index(0)]) == 1.0, name
    for a in range(3):
        leaf, pts, pose = CASES["q_edges_axis_%d" % a]
        q = M.point_terms(pts, pose, leaf, 0.0, 120.0)[3]
        assert set(q[:, a].tolist()) == {0, 65535}
    leaf, pts, pose = CASES["minus_1e_20"]
    _, v, _, q, _ = M.point_terms(pts, pose, leaf, 0.0, 120.0)
    assert v[0].tolist() == [-1, 3, 0] and q[0, 0] == 65535 and v[2].tolist() == [-1, -1, -1] and q[2].tolist() == [65535] * 3
    assert rec["negative_covariance"][0]["cov"][1] < 0.0
    assert rec["seen_from_below"][0]["normal"][2] == -1.0 and rec["seen_from_above"][0]["normal"][2] == 1.0
    m = model_of(*CASES["dot_zero_sensor_in_plane"])
    (e,) = m.vox.values()
    assert e[3][2] == 0 and rec["dot_zero_sensor_in_plane"][0]["normal"].tolist() == [0.0, 0.0, 1.0]
    tie = rec["plane_x_minus_y"][0]
    assert abs(tie["normal"][0]) == abs(tie["normal"][1]) > 0.7 and tie["normal"][2] == 0.0


def test_dot_zero_takes_the_sign_of_the_largest_component_and_the_lowest_axis_on_ties(program):
    """W = 0 makes every dot 0: random voxels (normals of either sign) and the plane whose normal has |n0| == |n1|"""
    rng = np.random.default_rng(31)
    m = model_of(0.5, rng.normal(size=(4000, 3)) * [2.0, 2.0, 0.5], None)
    entries = [[e[0], e[1], e[2], [0, 0, 0], e[4], e[5]] for e in m.vox.values() if e[4] >= 3]
    got = check_finish(program, entries, 0.5)
    big = np.abs(got["normal"]).argmax(axis=1)
    assert (got["normal"][np.arange(len(got)), big] > 0.0).all() and len(got) > 200
    flipped = sum(M.eigen([float(x) for x in r["cov"]])[1][b] < 0.0 for r, b in zip(got, big))
    assert 0 < flipped < len(got)  # the rule negated some and left others
    tie = model_of(*CASES["plane_x_minus_y"])
    (e,) = tie.vox.values()
    for mirror in (False, True):  # x - y = const and x + y = const
        S = list(e[2])
        s = list(e[1])
        if mirror:  # y -> 65535 - y per point: redo the sums from the points
            leaf, pts, pose = CASES["plane_x_minus_y"]
            q = M.point_terms(pts, pose, leaf, 0.0, 120.0)[3].astype(object)
            q[:, 1] = 65535 - q[:, 1]
            s = [int(sum(q[:, a])) for a in range(3)]
            S = [int(sum(q[:, a] * q[:, b])) for a, b in M.PAIRS]
        r = check_finish(program, [[e[0], s, S, [0, 0, 0], e[4], e[5]]], 1.0, mirror)[0]
        assert abs(r["normal"][0]) == abs(r["normal"][1]) and r["normal"][0] > 0.0, (mirror, r["normal"])  # axis 0 decides, not axis 1
        assert (r["normal"][1] < 0.0) == (not mirror)


def test_the_large_voxel_needs_the_128_bit_numerator(program):
    leaf, pts = M.big_voxel()
    m = model_of(leaf, pts, None)
    (e,) = m.vox.values()
    assert e[4] == 140000
    for k, (a, b) in enumerate(M.PAIRS):  # asserted on the model first: both count S and N are at least 2^64
        N, _ = M.numerator(e[4], e[2][k], e[1][a], e[1][b])
        assert e[4] * e[2][k] >= 1 << 64 and N >= 1 << 64, (k, N)
    r = check_finish(program, [e], leaf)[0]
    half = 65535.0 / 65536.0 / 2.0
    assert np.allclose(r["cov"], half * half, rtol=1e-12) and np.allclose(r["mean"], 4.0 + half, rtol=1e-15)
    # the largest sums the rule admits: 2^32 - 2 points, half of them at each end (synthetic sums)
    n = (1 << 32) - 2
    s = [(n // 2) * 65535] * 3
    S = [(n // 2) * 65535 * 65535] * 6
    assert max(S) < 1 << 64 and n * S[0] < 1 << 96
    check_finish(program, [[[0, 0, 0], s, S, [-(1 << 61), 1 << 61, 0], n, 0]], leaf, "largest sums")


def test_the_numerator_of_a_variance_is_never_negative_and_a_covariance_can_be():
    """count S[aa] >= s[a]^2 (Cauchy-Schwarz on integers) holds for every voxel of every case; N[ab] < 0 occurs"""
    rng = np.random.default_rng(32)
    sets = [model_of(*CASES[n]) for n in CASES] + [model_of(0.5, rng.uniform(-3, 3, (20000, 3)), None)]
    negative = 0
    for m in sets:
        for e in m.vox.values():
            for k, (a, b) in enumerate(M.PAIRS):
                N, f = M.numerator(e[4], e[2][k], e[1][a], e[1][b])
                assert a != b or (N >= 0 and f >= 0.0)
                assert (f < 0.0) == (N < 0)
                negative += N < 0
    assert negative > 100


def test_the_view_clamp_at_its_edges_and_with_an_infinite_quotient(program):
    C = 1 << 30
    leaf = 1.0
    step = leaf / 256.0
    # no rotation, the sensor at o: x = (o - p') / leaf * 256 with p' in the voxel at the origin
    p = np.array([[0.25, 0.25, 0.25]])
    for ox, want in ((C * step + 0.25, C), ((C - 1) * step + 0.25, C - 1), ((C + 5) * step + 0.25, C), (-C * step + 0.25, -C),
                     (-(C - 1) * step + 0.25, -(C - 1)), (-(C + 5) * step + 0.25, -C)):
        pose = np.array([0.0, 0, 0, 1.0, ox, 0.0, 0.0])
        # the point is given in the sensor frame so that p' = p + o lands on 0.25: p_sensor = 0.25 - ox
        ps = p - [ox, 0.0, 0.0]
        _, _, _, q, w = M.point_terms(ps, pose, leaf, 0.0, 1e12)
        assert w[0, 0] in (want, want - 1, want + 1) and abs(w[0, 0]) <= C, (ox, w[0])  # (p' is rounded: one step either way, never past the clamp)
        check_points(program, leaf, ps, pose, 0.0, 1e12)
    # a leaf so small that the quotient overflows: x is infinite, w the clamp
    tiny = 1e-300
    pose = np.array([0.0, 0, 0, 1.0, 1e10, -1e10, 0.0])
    ps = np.array([[-1e10, 1e10, 0.0]])  # p' = (0, 0, 0): voxel 0, and (o - p') / leaf overflows
    w = M.point_terms(ps, pose, tiny, 0.0, 1e12)[4]
    assert w[0].tolist() == [C, -C, 0]
    assert check_points(program, tiny, ps, pose, 0.0, 1e12) == 1
    assert M.view_terms([np.inf, -np.inf, np.nan], np.zeros((1, 3)), 1.0)[0].tolist() == [C, -C, -C]


@pytest.mark.parametrize("leaf", [0.1, 0.5, 1.0, 3.7])
def test_random_voxels_equal_the_model(program, leaf):
    rng = np.random.default_rng(int(leaf * 10))
    n_vox = 3000
    corners = rng.integers(-40, 40, (n_vox, 3))
    per = rng.integers(1, 12, n_vox)
    shape = rng.uniform(0.0, 1.0, (n_vox, 3)) ** 3  # thin, flat and round voxels
    pts = np.concatenate([(c + 0.5 + (rng.uniform(-0.5, 0.5, (k, 3)) * s)) * leaf for c, k, s in zip(corners, per, shape)])
    pts = pts[rng.permutation(len(pts))]
    pose = np.array([0.03, -0.02, 0.1, 0.99, 2.0, -1.0, 0.7])
    assert check_points(program, leaf, pts, pose, 0.5, 120.0 * max(leaf, 1.0)) > n_vox
    m = model_of(leaf, pts, pose, 0.5, 120.0 * max(leaf, 1.0))
    assert len(m.vox) >= 0.9 * n_vox
    check_finish(program, list(m.vox.values()), leaf, leaf)


def test_the_same_inputs_are_clean_under_asan_and_ubsan_in_the_stand_alone_program():
    san = M.hostcheck_program(san=True)
    for name in sorted(CASES):
        leaf, pts, pose = CASES[name]
        check_points(san, leaf, pts, pose)
        check_finish(san, list(model_of(leaf, pts, pose).vox.values()), leaf, name)
    leaf, pts = M.big_voxel()
    check_finish(san, list(model_of(leaf, pts, None).vox.values()), leaf)
    check_points(san, 1e-300, np.array([[-1e10, 1e10, 0.0], [np.nan, 0, 0], [1e200, 0, 0]]), np.array([0.0, 0, 0, 1.0, 1e10, -1e10, 0.0]), 0.0, 1e12)
