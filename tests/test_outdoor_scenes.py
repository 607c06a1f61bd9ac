"""CPU-only: the outdoor scenes of tests/outdoor_scenes.py produce what they exist for (large index cells, no-return beams,
returns beyond max_range, empty scan lines), and the host build of the kernels' math (tests/hostcheck) agrees with the oracle
on their feature sets: extraction index sequences, k-NN lists, registration."""
import numpy as np
import pytest

import hostcheck_lib as Hc
import outdoor_scenes as S

H, W = 64, 1024
PLANE_RADIUS = 2.0  # RegistrationParams().max_plane_neighbor_dist: the radius the plane index is chosen for


def _pdiff(O, a, b):
    d = O.pose_compose(O.pose_inverse(a), b)
    return O.quat_angular_distance(d[:4], [0, 0, 0, 1.0]), float(np.linalg.norm(d[4:]))


def test_scenes_are_deterministic():
    for name in S.SCENES:
        a, b = S.pair(name, 3), S.pair(name, 3)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        assert a[0].shape == (H * W, 3) and a[0].dtype == np.float64 and a[0].flags["C_CONTIGUOUS"]
    assert not np.array_equal(S.pair("lot", 3)[0], S.pair("lot", 4)[0])


# (name, smallest planar extent in x / y, cell edge at least)
SCENE_BARS = {"canyon": ((180.0, 30.0), 0.6), "lot": ((150.0, 150.0), 1.2), "field": ((120.0, 120.0), 1.2)}


@pytest.mark.parametrize("name", S.SCENES)
def test_scene_properties(oracle, name):
    (min_x, min_y), min_h = SCENE_BARS[name]
    tgt, src, motion = S.pair(name, 0)
    fwd, yaw = motion[4], 2 * np.arctan2(motion[2], motion[3])
    assert 0.3 <= fwd <= 1.5 and abs(yaw) <= np.radians(2.0) and not motion[5:].any()
    for scan in (tgt, src):
        r = np.linalg.norm(scan, axis=1)
        assert (r == 0).sum() > 100 and (r > 120.0).sum() > 20  # no-return beams and returns beyond max_range
        assert r.max() <= S.MAX_HIT + 0.1
    e, p = oracle.extract_features(tgt, H, W, 1.0, 120.0)
    ext = tgt[p].max(axis=0) - tgt[p].min(axis=0)
    assert ext[0] >= min_x and ext[1] >= min_y, ext
    h, dims = Hc.grid_choose(tgt[p], PLANE_RADIUS)
    assert h >= min_h, (h, dims)
    assert np.prod(dims) <= 65536
    lines = np.abs(tgt.reshape(H, W, 3)).sum(axis=(1, 2)) == 0
    if name == "field":
        # no enclosing walls: the lines above the tallest object see nothing at all, and the objects stand in a few
        # azimuth clusters, so sectors of lines that do see something hold few or no valid points
        assert lines.sum() >= 1 and lines[-1]
        r = np.linalg.norm(tgt, axis=1).reshape(H, W)
        valid = (r >= 1.0) & (r <= 120.0)
        sectors = np.stack([valid[:, s * W // 6:(s + 1) * W // 6].sum(axis=1) for s in range(6)], axis=1)  # (H, 6)
        assert ((sectors.max(axis=1) > 0) & (sectors.min(axis=1) < 10)).sum() >= 3
    else:
        assert not lines.any()


def test_room_keeps_its_half_metre_cells(oracle):
    A = Hc.synth_scan(1, 0, 0, H, W, 0.01)
    _, p = oracle.extract_features(A, H, W, 1.0, 120.0)
    assert Hc.grid_choose(A[p], PLANE_RADIUS)[0] == 0.5


@pytest.mark.parametrize("name", S.SCENES)
def test_host_extraction_on_outdoor_scans(oracle, name):
    fe, ofe = Hc.fe_params(), oracle.FeParams()
    for scan in S.pair(name, 1)[:2]:
        curv, mask = Hc.curvature_valid(scan, H, W, 1.0, 120.0, fe)
        assert np.array_equal(curv.view(np.uint64), oracle.compute_curvature(scan, H, W, ofe).view(np.uint64))
        assert np.array_equal(mask, oracle.compute_valid_points(scan, H, W, 1.0, 120.0, ofe))
        e, p = Hc.select(curv, mask, H, W, fe)
        oe, op = oracle.extract_features(scan, H, W, 1.0, 120.0, ofe)
        assert np.array_equal(e, oe) and np.array_equal(p, op)


@pytest.mark.parametrize("name", S.SCENES)
def test_host_knn_on_outdoor_feature_sets(oracle, name):
    """the keyed / queued / complete searches of the kernels (Hc.knn runs them all and counts disagreements) against
    brute force on scan-sized outdoor planar sets: queries are the source features moved by the true motion (inside
    the grid, dense blocks) and points far outside it"""
    rng = np.random.default_rng(5)
    tgt, src, motion = S.pair(name, 2)
    _, p = oracle.extract_features(tgt, H, W, 1.0, 120.0)
    _, ps = oracle.extract_features(src, H, W, 1.0, 120.0)
    pts = tgt[p]
    moved = np.array([oracle.pose_act(motion, x) for x in src[ps[rng.choice(len(ps), 400, replace=False)]]])
    q = np.concatenate([moved, pts[rng.integers(0, len(pts), 40)] + rng.normal(size=(40, 3)) * 2.0,
                        rng.uniform(-250.0, 250.0, (10, 3))])
    before = Hc.knn_mismatches()
    queued = Hc.knn_round2()[1]
    for k in (5, 8, 16):
        for radius in (2.0, -1.0):
            for i in range(len(q)):
                want = oracle.knn_bruteforce(pts, q[i], k, radius)
                assert np.array_equal(Hc.knn(pts, q[i], k, radius), want), (k, radius, i)
    assert Hc.knn_mismatches() == before == 0
    assert Hc.knn_round2()[1] > queued  # (the queue's searches ran)


@pytest.mark.parametrize("name", S.SCENES)
def test_host_registration_on_outdoor_pairs(oracle, name):
    tgt, src, _ = S.pair(name, 4)
    ea, pa = oracle.extract_features(tgt, H, W, 1.0, 120.0)
    eb, pb = oracle.extract_features(src, H, W, 1.0, 120.0)
    po, to, io = oracle.register_features(src[eb], src[pb], tgt[ea], tgt[pa])
    ph, th, ih = Hc.register(src[eb], src[pb], tgt[ea], tgt[pa])
    assert Hc.knn_mismatches() == 0
    assert (th, ih) == (to, io)
    rot, trans = _pdiff(oracle, po, ph)
    assert rot < 1e-12 and trans < 1e-12, (rot, trans)
