"""CPU-only: what the rule of the surfel map means, checked on the Python model alone (tests/surfel_common.py): the mean and the
covariance against numpy on the dequantised points, the eigenvalues and the normal's direction against numpy.linalg.eigh of that
covariance, and a wall and a floor ray-cast from tests/outdoor_scenes.py whose normals point back at the sensor.

The tolerances are measurements: measure() gives the largest deviation of the model from the numpy reference over this file's own
inputs (the values recorded below were measured with it), and the tests assert at eight times that, so that another BLAS or numpy
build does not trip them. Deviations are in units of the leaf (mean), of leaf^2 (covariance, eigenvalues) and plain (1 - |cos| of
the angle between the normals). The quantisation step leaf / 65536 = 1.5e-5 leaf is the floor for the mean against the ORIGINAL
points; against the dequantised points, which is what is compared here, only rounding is left."""
import numpy as np

import cloudmap_common as CM
import outdoor_scenes as S
import surfel_common as M

# measured by measure() (the largest deviation over inputs()): see DESIGN.md section 4.18
MEASURED = {"mean": 4.45e-15, "cov": 1.59e-15, "eval": 1.61e-15, "normal": 1.0e-15}
FACTOR = 8.0
GAP = 1e-3  # the normal is compared where the two smallest eigenvalues are at least this apart, relative to the largest


def inputs():
    """[(leaf, points, pose)]: random clouds at four leaves (round, flat and thin voxels), a far-away thin wall, and the lot scan"""
    rng = np.random.default_rng(418)
    out = []
    for leaf in (0.1, 0.5, 1.0, 3.7):
        pts = rng.normal(size=(6000, 3)) * np.array([6.0, 6.0, 0.6]) * leaf
        out.append((leaf, pts, np.array([0.03, -0.02, 0.1, 0.99, 2.0, -1.0, 0.7])))
    wall = np.stack([np.full(4000, 99.73), rng.uniform(-2, 2, 4000), rng.uniform(0, 2, 4000)], axis=1) + rng.normal(size=(4000, 3)) * [0.004, 0, 0]
    out.append((0.5, wall, None))
    origin, yaw = S.sensor_origin("lot", 0)
    out.append((2.0, S.scan_at("lot", 0, origin, yaw, H=32, W=512), S.yaw_pose(yaw, origin)))
    return out


def dequantised(leaf, pts, pose, min_range=0.5, max_range=120.0):
    """{key: (n, 3) float64} the points as the map sees them: (v + q / 65536) leaf"""
    what, v, key, q, _ = M.point_terms(np.asarray(pts, dtype=np.float64), pose, leaf, min_range, max_range)
    used = what == CM.USED
    x = (v[used].astype(np.float64) + q[used].astype(np.float64) / M.UNIT) * leaf
    groups = {}
    for k, row in zip(key[used].tolist(), x):
        groups.setdefault(k, []).append(row)
    return {k: np.array(g) for k, g in groups.items()}


def deviations(leaf, pts, pose):
    """the largest deviation of the model's records from numpy on the dequantised points of one input, per quantity"""
    model = M.SurfelMapModel(leaf, 0.5, 120.0)
    model.add(pts, poses=None if pose is None else pose[None])
    rec, _ = model.emit()
    groups = dequantised(leaf, pts, pose)
    assert list(groups) == list(model.vox)  # (the same voxels in the same order)
    dev = {"mean": 0.0, "cov": 0.0, "eval": 0.0, "normal": 0.0}
    compared = 0
    for r, x in zip(rec, groups.values()):
        assert len(x) == r["count"]
        centre = np.floor(x[0] / leaf) * leaf  # (numpy's own sums are taken about the voxel's corner, where they are well conditioned)
        y = x - centre
        mean = y.mean(axis=0)
        c = (y - mean).T @ (y - mean) / len(y)
        dev["mean"] = max(dev["mean"], np.abs(r["mean"] - (mean + centre)).max() / leaf)
        cov = np.array([[r["cov"][0], r["cov"][1], r["cov"][2]], [r["cov"][1], r["cov"][3], r["cov"][4]], [r["cov"][2], r["cov"][4], r["cov"][5]]])
        dev["cov"] = max(dev["cov"], np.abs(cov - c).max() / leaf ** 2)
        w, vec = np.linalg.eigh(c)
        dev["eval"] = max(dev["eval"], np.abs(r["eval"] - w).max() / leaf ** 2)
        if len(x) >= 4 and w[1] - w[0] > GAP * w[2]:
            dev["normal"] = max(dev["normal"], 1.0 - abs(float(np.dot(vec[:, 0], r["normal"]))))
            compared += 1
    return dev, compared, len(rec)


def measure():
    total = {"mean": 0.0, "cov": 0.0, "eval": 0.0, "normal": 0.0}
    for leaf, pts, pose in inputs():
        dev, compared, n = deviations(leaf, pts, pose)
        assert compared > 20 and n >= 32, (leaf, compared, n)
        for k in total:
            total[k] = max(total[k], dev[k])
    return total


def test_mean_covariance_eigenvalues_and_normal_against_numpy_within_eight_times_the_measured_deviation():
    got = measure()
    print("\n[surfel model against numpy] " + ", ".join(f"{k} {got[k]:.3g} (bound {FACTOR * MEASURED[k]:.3g})" for k in got))
    for k in got:
        assert got[k] <= FACTOR * MEASURED[k], (k, got[k], MEASURED[k])
    assert MEASURED["mean"] < 1.0 / M.UNIT  # far below the quantisation step, the floor against the original points


def test_the_mean_is_within_one_quantisation_step_of_the_original_points_mean():
    rng = np.random.default_rng(419)
    leaf = 0.5
    pts = rng.normal(size=(5000, 3)) * [3.0, 3.0, 0.3]
    model = M.SurfelMapModel(leaf, 0.0, 120.0)
    model.add(pts)
    rec, _ = model.emit()
    ok, v, _ = CM.cells(pts, leaf)
    key = CM.pack(v)
    for r, k in zip(rec, model.vox):
        exact = pts[key == np.uint64(k)].mean(axis=0)
        d = exact - r["mean"]
        assert (d >= -1e-12).all() and (d < leaf / M.UNIT + 1e-12).all()  # offsets are floored: the mean lies below by less than a step


def test_a_thin_wall_far_from_the_voxels_corner_keeps_its_thickness():
    """the case S / n - mean^2 in FP64 would lose: the spread across the wall is 4 mm in a voxel 100 m from the origin"""
    leaf, wall, _ = inputs()[4]
    model = M.SurfelMapModel(leaf, 0.5, 120.0)
    model.add(wall)
    rec, _ = model.emit(20)
    assert len(rec) == 32  # (8 x 4 voxels of the wall's plane, about 125 points each)
    sigma = np.sqrt(rec["eval"][:, 0])
    assert (np.abs(np.abs(rec["normal"][:, 0]) - 1.0) < 1e-3).all() and (rec["normal"][:, 0] < 0).all()  # facing the origin
    assert 0.002 < np.median(sigma) < 0.006 and (rec["eval"][:, 0] >= 0.0).all()


def test_a_ray_cast_wall_and_floor_point_back_at_the_sensor():
    boxes = [np.array([[10.5, -30.0, 0.0], [11.5, 30.0, 12.0]])]  # one wall 10.5 m ahead, inside its voxels; the ground is the scene's own
    origin = np.array([0.0, 0.0, S.SENSOR_HEIGHT])
    scan = S.cast(boxes, origin, 0.0, 32, 512, S.FANS["lot"], 0.01, np.random.default_rng(3))
    pose = S.yaw_pose(0.0, origin)
    model = M.SurfelMapModel(1.0, 0.5, 60.0)
    model.add(scan, poses=pose[None])
    rec, _ = model.emit(8)
    mean, normal = rec["mean"], rec["normal"]
    wall = (np.abs(mean[:, 0] - 10.5) < 0.1) & (mean[:, 2] > 1.0)  # (the lowest row of wall voxels holds ground as well)
    floor = (mean[:, 2] < 0.1) & (mean[:, 0] < 9.5)
    assert wall.sum() > 10 and floor.sum() > 20
    assert (normal[wall, 0] < -0.99).all()      # the wall's outward normal is -x: back at the sensor
    assert (normal[floor, 2] > 0.99).all()      # the floor's is +z
    to_sensor = origin[None, :] - mean
    assert ((normal * to_sensor).sum(axis=1)[wall | floor] > 0.0).all()
    assert (rec["eval"][wall | floor, 0] < 0.05 * rec["eval"][wall | floor, 2]).all()  # flat
    # the signed distance of the sensor to a wall voxel's plane is the 10.5 m in front of it
    near = np.flatnonzero(wall & (np.abs(mean[:, 1]) < 1.0))
    assert len(near) and all(abs(M.distance((rec[i]["mean"].tolist(), None, None, rec[i]["normal"].tolist()), origin) - 10.5) < 0.05 for i in near)


def test_the_model_map_keeps_order_of_first_appearance_counts_every_drop_and_both_claims():
    m = M.SurfelMapModel(1.0, 0.5, 10.0)
    pts = np.array([[2.5, 0, 0], [1.5, 0, 0], [2.25, 0, 0], [0, 0, 0], [np.nan, 0, 0], [11, 0, 0], [1.75, 0.5, 0]])
    m.add(pts)
    m.add(np.array([[3.5, 0, 0], [2.75, 0, 0]]), poses=np.array([[0, 0, 0, 1.0, 0, 0, 0]]))
    rec, n = m.emit()
    assert n == 3 and rec["first"].tolist() == [0, 1, 7] and rec["count"].tolist() == [3, 2, 1]
    assert rec["mean"].tolist() == [[2.5, 0.0, 0.0], [1.625, 0.25, 0.0], [3.5, 0.0, 0.0]]
    assert m.stats() == dict(voxels=3, points_offered=9, points_used=6, invalid=1, range=2, outside=0, overflow=0)
    assert m.emit(2)[1] == 2 and m.emit(1, capacity=1)[0]["first"].tolist() == [0]
    assert (m.plain_claims, m.wave_claims) == (6, 6)  # no two neighbours share a voxel
    rec_q, dist, cnt = m.query(np.array([[2.9, 0.1, 0.1], [7.0, 7.0, 7.0], [1.1, 0.9, 0.0]]), 2)
    assert cnt.tolist() == [3, 0, 2] and dist[1] == 0.0 and not rec_q[1].tobytes().strip(b"\0")
