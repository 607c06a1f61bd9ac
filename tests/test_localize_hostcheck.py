"""CPU-only: localize_math.h — the rule of the surfel localisation kernels (loam_amd/csrc/localize_kernels.hip) — compiled with g++
together with a host loop that runs the whole solve in the kernels' orders (tests/hostcheck_localize), against the independent numpy
model of tests/localize_common.py. Discrete outputs by equality: the chosen candidate of every point, every counter, used_mask,
termination, iterations. Floats within 8 x the largest deviation measured over this file's own inputs (the policy of
tests/test_surfel_model.py). The GPU tests (test_gpu_localize.py) compare the kernels with the same host build by bytes. The last
test runs the same inputs through the stand-alone program built with AddressSanitizer + UndefinedBehaviorSanitizer.

MEASURED (this file's inputs, host build against the numpy model; deviation() below defines the figures):
    largest float deviation  4.74e-15  (the canyon scene from 0.2 m / 1.5 degrees, neighbourhood 7)  -> FLOAT_TOL = 8 x 4.8e-15
    pose error of the host build at the returned pose, scan 7 of the 16 x 256 drives from 0.2 m / 1.5 degrees, neighbourhood 7:
        lot     0.0158 m / 0.0116 degrees (4 iterations)   canyon  0.0462 m / 0.0228 degrees (3 iterations)  -> POSE_BOUND = 2 x these
    (what six noisy 16-line scans at leaf 0.5 m leave of a plane per voxel; the canyon's error lies along the street. Home voxel
    only: lot 0.0074 m / 0.0109 degrees, canyon 0.0027 m / 0.0421 degrees, 3 iterations each, asserted at 2 x as well. Leaf 1.0 m from 0.4 m / 3 degrees on
    the lot: 0.0099 m / 0.0084 degrees.)"""
import numpy as np
import pytest

import localize_common as L

FLOAT_TOL = 8 * 4.8e-15
POSE_BOUND = {("lot", 7): (2 * 0.0158, 2 * 0.0116), ("canyon", 7): (2 * 0.0462, 2 * 0.0228),
              ("lot", 1): (2 * 0.0074, 2 * 0.0109), ("canyon", 1): (2 * 0.0027, 2 * 0.0421)}
MICRO = L.micro_cases()
BITS = np.uint64


def deviation(h, c, res, ev):
    """the largest of: |pose - pose| (absolute), the two costs (relative), H against its largest entry, the gradient against
    sqrt(H_ii cost), the eigenvalues against the largest; host record c against the model's (res, ev)"""
    r, info = h["results"][c], h["info"][c]
    d = [float(np.abs(h["poses"][c] - res["pose"]).max()) if np.isfinite(res["pose"]).all() else 0.0]
    for name in ("initial_cost", "final_cost"):
        d.append(abs(float(r[name]) - res[name]) / max(abs(res[name]), 1e-300))
    Hm = ev["H"]
    if ev["n_rows"]:
        d.append(float(np.abs(info["information"] - Hm).max() / np.abs(Hm).max()))
        scale = np.sqrt(np.diag(Hm) * max(ev["cost"], 1e-300)) + 1e-300
        d.append(float((np.abs(info["gradient"] - ev["g"]) / scale).max()))
        d.append(float(np.abs(info["eigenvalues"] - res["eigenvalues"]).max() / np.abs(res["eigenvalues"]).max()))
    return max(d)


def check_against_model(model, pts, pose, p, what, program=None):
    """one cloud through the host build and the numpy model; returns (host outputs, model result, the deviation)"""
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    h = L.host_run(model, pts, [0, len(pts)], np.asarray(pose)[None], p, program)
    T, res, ev = L.LocalizeModel(model, p).solve(pts, pose)
    near = ev["near"]
    assert near.mean() <= 0.01 if len(pts) > 100 else True, (what, int(near.sum()))  # at most 1 % of a case's points are left out
    assert np.array_equal(h["chosen"][~near], ev["chosen"][~near]), (what, np.flatnonzero(h["chosen"] != ev["chosen"])[:10])
    # On this file's fixed inputs NO point lies that close to a decision, so nothing is left out and everything below is compared on
    # every point. An input that brings a near point has to be compared without it; it must not pass by comparing less.
    assert not near.any(), (what, "points within 1e-9 of a decision", np.flatnonzero(near)[:10])
    r = h["results"][0]
    for name in L.DISCRETE:
        assert int(r[name]) == int(res[name]), (what, name, int(r[name]), int(res[name]))
    assert L.CM.same_bytes(h["poses"][0], np.ascontiguousarray(r["pose"])), what
    info = h["info"][0]
    assert info["n_edge"] == 0 and info["n_plane"] == r["n_rows"] and info["n_huber"] == r["n_huber"] and info["n_dropped"] == 0
    assert info["weighted_sq_error"].view(BITS) == r["final_cost"].view(BITS)
    assert np.array_equal(info["information"].view(BITS), info["information"].T.copy().view(BITS))  # bitwise symmetric
    assert len(pts) == sum(int(r[k]) for k in ("n_rows", "n_no_surfel", "n_gated", "n_unused")), what
    dev = deviation(h, 0, res, ev)
    print(f"{what}: deviation {dev:.3g}")
    assert dev <= FLOAT_TOL, (what, dev)
    return h, res, dev


@pytest.mark.parametrize("name", sorted(MICRO))
def test_candidate_and_gate_case(name):
    model, pts, pose, p, want = MICRO[name]
    h = L.host_run(model, pts, [0, len(pts)], pose[None], p)
    T, res, ev = L.LocalizeModel(model, p).solve(pts, pose)
    assert h["chosen"].tolist() == ev["chosen"].tolist(), name  # (by equality even where two decisions meet: the cases are exact)
    if want is not None:
        assert h["chosen"].tolist() == want, (name, h["chosen"])
    r = h["results"][0]
    for k in L.DISCRETE:
        assert int(r[k]) == int(res[k]), (name, k)
    assert r["iterations"] == 0 and r["termination"] == L.MAX_ITERATIONS and L.CM.same_bytes(h["poses"][0], pose)
    assert abs(float(r["final_cost"]) - res["final_cost"]) <= FLOAT_TOL * max(res["final_cost"], 1.0)


def test_what_the_named_cases_are_there_for():
    """each case reaches the path its name promises (asserted on the model's voxels)"""
    from surfel_common import finish
    def records(m):
        return {tuple(e[0]): finish(e[0], e[1], e[2], e[3], e[4], e[5], m.leaf) for e in m.vox.values()}
    rec = records(MICRO["home_below_min_points_7"][0])
    assert rec[(6, 5, 5)][4] == 3 and rec[(5, 5, 5)][4] == 16
    cube = records(MICRO["home_a_cube_lattice"][0])[(6, 5, 5)]
    assert cube[2][0] == cube[2][1] == cube[2][2] > 0.0  # three equal eigenvalues: eval[0] <= 0.1 eval[1] fails
    line = records(MICRO["home_a_line_along_x"][0])[(6, 5, 5)]
    assert line[2][0] == 0.0 and line[2][1] == 0.0 and line[2][2] > 0.0  # eval[1] > 0 fails
    diag = records(MICRO["home_a_diagonal_line"][0])[(6, 5, 5)]
    assert abs(diag[2][1]) < 1e-12 * diag[2][2]
    m, pts, _, _, _ = MICRO["tie_minus_x_before_plus_x"]
    a, b = records(m)[(5, 5, 5)], records(m)[(7, 5, 5)]
    assert a[0] == [5.5, 5.5, 5.5] and b[0] == [7.5, 5.5, 5.5] and (6, 5, 5) not in records(m)
    d2 = [sum((float(pts[0][k]) - r[0][k]) ** 2 for k in range(3)) for r in (a, b)]
    assert d2[0] == d2[1]
    m, pts, _, p, _ = MICRO["s_at_max_distance"]
    fl = records(m)[(5, 5, 5)]
    assert fl[0][2] == 5.5 and [abs(x) for x in fl[3]] == [0.0, 0.0, 1.0]
    assert pts[0][2] - 5.5 == p["max_distance"] == 5.5 - pts[2][2] and pts[1][2] - 5.5 > p["max_distance"]
    h = L.host_run(m, pts, [0, 4], L.IDENTITY[None], MICRO["s_at_huber_delta"][3])
    assert h["results"][0]["n_huber"] == 2  # exactly at huber_delta: not scaled; one unit in the last place beyond: scaled
    assert L.host_run(m, pts, [0, 4], L.IDENTITY[None], MICRO["huber_off"][3])["results"][0]["n_huber"] == 0


def test_candidate_keys_and_the_skip_at_the_edge_of_the_voxel_range():
    """loc_candidate_key itself: the six face neighbours in the order -x +x -y +y -z +z, and false where a coordinate would leave
    |v| < 2^20 (biased 1 and 2^21 - 1), on each axis; a missing bound check would wrap into the neighbouring field of the key"""
    top = (1 << 20) - 1
    steps = [(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]

    def pack(v):
        return int(L.CM.pack(np.array([v], dtype=np.int64))[0])

    for home in ((5, -7, 11), (0, 0, 0), (-3, top - 1, -top + 1)):
        for k, d in enumerate(steps):
            assert L.candidate_key(pack(home), k) == (True, pack(tuple(a + b for a, b in zip(home, d)))), (home, k)
    for axis in range(3):
        for edge, k_out, k_in in ((top, 2 + 2 * axis, 1 + 2 * axis), (-top, 1 + 2 * axis, 2 + 2 * axis)):
            home = [4, -9, 13]
            home[axis] = edge
            assert L.candidate_key(pack(home), k_out)[0] is False, (axis, edge)
            inner = list(home)
            inner[axis] = edge - (1 if edge > 0 else -1)
            assert L.candidate_key(pack(home), k_in) == (True, pack(inner)), (axis, edge)
            assert L.candidate_key(pack(home), 0) == (True, pack(home))


def test_floor_only_map_moves_z_roll_and_pitch_only():
    m, pts, truth = L.floor_map()
    p = L.params(min_eigenvalue_per_row=0.01)
    cloud = pts[::7]
    init = L.displaced(truth, 0.1, 1.0, seed=3)
    T, res, ev = L.LocalizeModel(m, p).solve(cloud, init)
    per_row = res["eigenvalues"] / res["n_rows"]  # asserted on the model first
    assert (per_row[:3] < 0.01).all() and (per_row[3:] > 0.01).all(), per_row
    h, res, _ = check_against_model(m, cloud, init, p, "floor")
    r, info = h["results"][0], h["info"][0]
    assert r["used_mask"] == 0b111000 and r["termination"] == L.CONVERGED
    used = np.abs(info["eigenvectors"][3:])
    assert (used[:, [2, 3, 4]] < 1e-2).all()  # yaw and the two translations in the plane take no part
    assert abs(h["poses"][0][6] - truth[6]) < 5e-3 and abs(init[6] - truth[6]) > 2e-2  # the height is found again


def test_empty_map_has_too_few_rows_and_keeps_the_pose():
    import surfel_common as M
    m = M.SurfelMapModel(0.5, 0.5, 120.0)
    scans, poses = L.drive("lot")
    init = L.displaced(poses[6])
    h, res, _ = check_against_model(m, scans[6], init, L.params(), "empty map")
    r = h["results"][0]
    assert r["termination"] == L.TOO_FEW_ROWS and r["iterations"] == 0 and r["n_rows"] == 0 and L.CM.same_bytes(h["poses"][0], init)
    assert r["n_no_surfel"] + r["n_unused"] == len(scans[6]) and not h["info"][0]["information"].any()


def test_max_iterations_0_returns_the_pose_and_the_information_at_it():
    scans, poses = L.drive("lot")
    init = L.displaced(poses[6])
    h, res, _ = check_against_model(L.drive_map("lot"), scans[6], init, L.params(max_iterations=0), "max_iterations 0")
    r = h["results"][0]
    assert r["iterations"] == 0 and r["termination"] == L.MAX_ITERATIONS and L.CM.same_bytes(h["poses"][0], init)
    assert r["n_rows"] == r["n_rows_initial"] > 1500 and r["initial_cost"].view(BITS) == r["final_cost"].view(BITS)


def test_nan_pose_is_not_finite():
    scans, poses = L.drive("lot")
    for k in (0, 3, 5):
        init = poses[6].copy()
        init[k] = np.nan
        h = L.host_run(L.drive_map("lot"), scans[6], [0, len(scans[6])], init[None], L.params())
        r = h["results"][0]
        assert r["termination"] == L.NOT_FINITE and r["iterations"] == 0 and L.CM.same_bytes(h["poses"][0], init), k
        T, res, ev = L.LocalizeModel(L.drive_map("lot"), L.params()).solve(scans[6], init)
        assert res["termination"] == L.NOT_FINITE and int(r["n_rows"]) == res["n_rows"] == 0


def test_non_unit_quaternion_is_used_as_given():
    scans, poses = L.drive("lot")
    init = L.displaced(poses[6]) * np.array([1.02, 1.02, 1.02, 1.02, 1.0, 1.0, 1.0])
    h, res, _ = check_against_model(L.drive_map("lot"), scans[6], init, L.params(), "non-unit quaternion")
    assert h["results"][0]["iterations"] >= 1 and h["results"][0]["n_rows"] > 1000


@pytest.mark.parametrize("name", ["lot", "canyon"])
@pytest.mark.parametrize("neighborhood", [7, 1])
def test_convergence_from_20_cm_and_1_5_degrees(name, neighborhood):
    scans, poses = L.drive(name)
    init = L.displaced(poses[6])
    assert abs(L.pose_error(init, poses[6])[0] - 0.2) < 1e-9 and abs(L.pose_error(init, poses[6])[1] - 1.5) < 1e-6
    p = L.params(neighborhood=neighborhood)
    h, res, _ = check_against_model(L.drive_map(name), scans[6], init, p, f"{name} {neighborhood}")
    r = h["results"][0]
    err = L.pose_error(h["poses"][0], poses[6])
    print(f"{name} neighbourhood {neighborhood}: {int(r['iterations'])} iterations, error {err[0]:.4f} m / {err[1]:.4f} degrees, rows {int(r['n_rows'])}")
    assert r["termination"] == L.CONVERGED and r["iterations"] <= p["max_iterations"]
    assert r["used_mask"] == 63 and r["final_cost"] < r["initial_cost"]
    bound = POSE_BOUND[(name, neighborhood)]
    assert err[0] <= bound[0] and err[1] <= bound[1], (err, bound)


def test_leaf_1_m_from_40_cm_and_3_degrees():
    scans, poses = L.drive("lot")
    init = L.displaced(poses[6], 0.4, 3.0, seed=1)
    h, res, _ = check_against_model(L.drive_map("lot", leaf=1.0), scans[6], init, L.params(), "lot leaf 1.0")
    err = L.pose_error(h["poses"][0], poses[6])
    print(f"leaf 1.0: error {err[0]:.4f} m / {err[1]:.4f} degrees")
    assert h["results"][0]["termination"] == L.CONVERGED and err[0] < 0.05 and err[1] < 0.05


def test_a_batch_equals_its_clouds_alone_and_stops_cloud_by_cloud():
    """one converged, one at the cap, one with too few rows, one not finite, and an empty cloud, in one call"""
    scans, poses = L.drive("lot")
    m = L.drive_map("lot")
    p = L.params(max_iterations=3)
    bad = poses[6].copy()
    bad[4] = np.inf
    clouds = [scans[6], scans[6], scans[6][:120], scans[6][:0], scans[6]]
    inits = np.stack([L.displaced(poses[6], 0.02, 0.1), L.displaced(poses[6], 0.6, 4.0, seed=2), poses[6], poses[6], bad])
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    h = L.host_run(m, np.concatenate(clouds), off, inits, p)
    assert h["results"]["termination"].tolist() == [L.CONVERGED, L.MAX_ITERATIONS, L.TOO_FEW_ROWS, L.TOO_FEW_ROWS, L.NOT_FINITE]
    assert h["results"]["iterations"].tolist()[1:] == [3, 0, 0, 0] and 1 <= h["results"]["iterations"][0] < 3
    for c in range(5):
        alone = L.host_run(m, clouds[c], [0, len(clouds[c])], inits[c][None], p)
        assert L.CM.same_bytes(alone["results"], h["results"][c:c + 1]) and L.CM.same_bytes(alone["info"], h["info"][c:c + 1]), c


def test_the_same_inputs_are_clean_under_asan_and_ubsan_in_the_stand_alone_program():
    san = L.hostcheck_san_program()
    for name in sorted(MICRO):
        model, pts, pose, p, _ = MICRO[name]
        a, b = L.host_run(model, pts, [0, len(pts)], pose[None], p), L.host_run(model, pts, [0, len(pts)], pose[None], p, san)
        assert all(L.CM.same_bytes(a[k], b[k]) for k in a), name
    scans, poses = L.drive("lot")
    m = L.drive_map("lot")
    bad = poses[6].copy()
    bad[0] = np.nan
    clouds = [scans[6], scans[6][:0], scans[6][:4097], scans[6]]
    inits = np.stack([L.displaced(poses[6]), poses[6], poses[6], bad])
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    a, b = L.host_run(m, np.concatenate(clouds), off, inits, L.params()), L.host_run(m, np.concatenate(clouds), off, inits, L.params(), san)
    assert all(L.CM.same_bytes(a[k], b[k]) for k in a)
