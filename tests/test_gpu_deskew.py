"""GPU: loamx_deskew_scans_dev[_f32] (include/loamx.h, "scan sequences"): per-point motion correction of a batch of scans.

Convention under test: scans are row-major [line][column], column c was measured at sweep fraction tau = c / W;
motion = (q, t) = start_T_end of the sweep, q normalised and taken along the short arc; T(tau) = (slerp(identity, q, tau),
tau t); p_out = R(rho)^T (R(tau) p + (tau - rho) t). Points that are exactly zero or not finite are left as they are."""
import numpy as np
import pytest

import sequence_common as Q
from gpu_common import ctx
from loam_amd import capi

pytestmark = pytest.mark.gpu

H, W, N = Q.H, Q.W, Q.N
IDENT = np.array([0, 0, 0, 1.0, 0, 0, 0])


def rotation_matrices(q):
    """(n, 4) unit quaternions (x, y, z, w) -> (n, 3, 3), the formula of Pose3d::matrix (include/loam/geometry.h)"""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.stack([np.stack([1 - (tyy + tzz), txy - twz, txz + twy], -1), np.stack([txy + twz, 1 - (txx + tzz), tyz - twx], -1),
                     np.stack([txz - twy, tyz + twx, 1 - (txx + tyy)], -1)], -2)


def slerp_from_identity(q, tau):
    """unit q (w >= 0), tau (n,) -> (n, 4): (sin(tau theta / 2) v / |v|, cos(tau theta / 2)), theta = 2 atan2(|v|, w);
    |v| < 1e-12: (tau v, 1) normalised"""
    v, vn = q[:3], np.linalg.norm(q[:3])
    if vn < 1e-12:
        out = np.concatenate([tau[:, None] * v[None, :], np.ones((len(tau), 1))], axis=1)
        return out / np.linalg.norm(out, axis=1, keepdims=True)
    half = tau * np.arctan2(vn, q[3])
    return np.concatenate([np.sin(half)[:, None] * (v / vn)[None, :], np.cos(half)[:, None]], axis=1)


def deskew_numpy(scan, motion, rho, h, w):
    """FP64 restatement of the convention; scan (h * w, 3) float64"""
    q = motion[:4] / np.linalg.norm(motion[:4])
    if q[3] < 0:
        q = -q
    t = motion[4:]
    tau = np.arange(w) / w
    Rt = rotation_matrices(slerp_from_identity(q, tau))                # (w, 3, 3)
    Rr = rotation_matrices(slerp_from_identity(q, np.array([rho])))[0]
    p = scan.reshape(h, w, 3)
    moved = np.einsum("cij,lcj->lci", Rt, p) + ((tau - rho)[:, None] * t[None, :])[None, :, :]
    out = np.einsum("ji,lcj->lci", Rr, moved)
    keep = (p == 0).all(axis=2) | ~np.isfinite(p).all(axis=2)
    out[keep] = p[keep]
    return out.reshape(-1, 3)


def bound(p, t):
    """|error| allowed per point: 1e-12 (1 + |p| + |t|) m — about 30 roundings and few-ulp libm differences, ~100x margin"""
    return 1e-12 * (1.0 + np.linalg.norm(p, axis=-1) + np.linalg.norm(t))


def check_points(got, want, src, t, where):
    live = np.isfinite(src).all(axis=1) & ~(src == 0).all(axis=1)
    err = np.linalg.norm(got[live] - want[live], axis=1)
    lim = bound(src[live], t)
    print(where, "max error", err.max(), "m; tightest allowance", lim.min(), "worst ratio", (err / lim).max())
    assert (err <= lim).all(), (where, err.max())
    assert np.array_equal(got[~live].view(np.uint64), src[~live].view(np.uint64)), where  # (zeros stay zero bitwise)


def sequence_motions():
    """the first three results of canyon-9 as sweep motions (scan p_T_scan p + 1 is what a constant-velocity sweep moved by)"""
    name, n = Q.SEQUENCES[0]
    scans = Q.sequence(name, n)
    res = Q.sequence_dev(ctx(), scans[:4])
    return scans, np.ascontiguousarray(res["pose"][:3])


def test_identity_motion_returns_the_input_bit_for_bit():
    c = ctx()
    scans = Q.sequence(*Q.SEQUENCES[0])[:2].copy()
    scans[1, 777] = [np.nan, 1.0, 2.0]        # (copied unchanged)
    scans[1, 778] = [3.0, -np.inf, 2.0]
    assert ((scans[0] == 0).all(axis=1)).sum() > 100  # (no-return beams are part of the input)
    motions = np.tile(IDENT, (2, 1))
    motions[1, :4] = [0, 0, 0, -2.5]  # (the identity rotation, neither normalised nor on the short arc)
    for rho in (0.0, 0.3, 1.0):
        for data in (scans, scans.astype(np.float32)):
            bits = np.uint64 if data.dtype == np.float64 else np.uint32
            got = c.deskew_scans(data, Q.lidar(), motions, rho)  # in place on the device
            assert got.dtype == data.dtype and np.array_equal(got.view(bits), data.view(bits)), (rho, data.dtype)
            d_in, d_out, d_m = c.alloc(data.nbytes).upload(data), c.alloc(data.nbytes), c.alloc(motions.nbytes).upload(motions)
            c.deskew_scans_dev(d_in.ptr, 2, Q.lidar(), d_m.ptr, d_out.ptr, rho, f32=data.dtype == np.float32)
            c.synchronize()
            assert np.array_equal(d_out.download(bits, data.size), data.view(bits).reshape(-1)), (rho, data.dtype, "out of place")
            assert np.array_equal(d_in.download(bits, data.size), data.view(bits).reshape(-1))
            for b in (d_in, d_out, d_m):
                b.free()


def test_formula_parity():
    """three scans of canyon-9 with the sequence's own results as motions, rho in {0, 0.5, 1}; a motion given with w < 0 and
    one with |v| = 1e-14. FP64 form: every finite non-zero point within 1e-12 (1 + |p| + |t|) m of the numpy restatement.
    FP32 form: equal to the FP64 form's result on the widened scans rounded to float, within 1 ulp of float per coordinate
    (it is the same arithmetic with one rounding on store), and within the FP64 allowance plus that rounding of numpy.
    Not asserted: numpy's OWN result rounded to float, per coordinate. The ray caster leaves coordinates of 1e-16 m in the
    column that looks along the x axis (y = r sin(0 + rounding)); there two FP64 evaluations in different operation order
    differ by ~1e-17 m, far inside any FP64 bound and thousands of float ulps of such a value. Measured on the MI355X:
    at rho = 0.5, 174 of 589 824 coordinates (all below 2.3e-14 m in magnitude) differ from numpy's rounded result by more
    than an ulp, the largest difference 1.1e-16 m; every other coordinate, and every coordinate at rho = 0 and 1, is within
    one ulp. The test prints these figures."""
    c = ctx()
    scans, motions = sequence_motions()
    batch = np.ascontiguousarray(scans[1:4])
    cases = [("sequence", motions)]
    neg = motions.copy()
    neg[:, :4] *= -3.0  # (w < 0 and not normalised: the same rotations)
    cases.append(("w<0", neg))
    tiny = motions.copy()
    tiny[:, :4] = [[1e-14, 0, 0, 1.0], [0, 6e-15, 8e-15, 1.0], [0, 0, -1e-14, 1.0]]
    cases.append(("|v|=1e-14", tiny))
    for what, m in cases:
        for rho in (0.0, 0.5, 1.0):
            got = c.deskew_scans(batch, Q.lidar(), m, rho)
            want = np.stack([deskew_numpy(batch[s], m[s], rho, H, W) for s in range(3)])
            for s in range(3):
                check_points(got[s], want[s], batch[s], m[s, 4:], (what, rho, s))
            if what == "w<0":  # (the same motion as "sequence")
                ref = np.stack([deskew_numpy(batch[s], motions[s], rho, H, W) for s in range(3)])
                for s in range(3):
                    check_points(got[s], ref[s], batch[s], m[s, 4:], (what, rho, s, "against q"))
            b32 = np.ascontiguousarray(batch.astype(np.float32))
            wide = b32.astype(np.float64)
            got32 = c.deskew_scans(b32, Q.lidar(), m, rho)
            assert got32.dtype == np.float32
            # (a) the FP64 form on the widened scans, rounded to float: the same arithmetic, one rounding on store
            dev32 = c.deskew_scans(wide, Q.lidar(), m, rho).astype(np.float32)
            ulp = np.spacing(np.abs(dev32)).astype(np.float64)
            diff = np.abs(got32.astype(np.float64) - dev32.astype(np.float64))
            print(what, rho, "f32 against the FP64 form rounded: coordinates that differ", int((diff > 0).sum()), "by more than an ulp", int((diff > ulp).sum()))
            assert (diff <= ulp).all(), (what, rho)
            # (b) the numpy restatement: the FP64 allowance of every point plus the rounding of the store
            want64 = np.stack([deskew_numpy(wide[s], m[s], rho, H, W) for s in range(3)])
            for s in range(3):
                live = ~(b32[s] == 0).all(axis=1)
                err = np.linalg.norm(got32[s][live].astype(np.float64) - want64[s][live], axis=1)
                lim = bound(wide[s][live], m[s, 4:]) + np.linalg.norm(np.spacing(np.abs(want64[s][live]).astype(np.float32)).astype(np.float64), axis=1)
                assert (err <= lim).all(), (what, rho, s, "f32 against numpy")
            # the figure of the stricter reading (numpy's result rounded to float, per coordinate): reported, see the docstring
            w32 = want64.astype(np.float32)
            u = np.spacing(np.abs(w32)).astype(np.float64)
            d = np.abs(got32.astype(np.float64) - w32.astype(np.float64))
            off = d > u
            print(what, rho, "f32 against numpy rounded, per coordinate: more than an ulp off", int(off.sum()), "largest such coordinate",
                  float(np.abs(w32[off]).max()) if off.any() else 0.0, "m, largest difference", float(d[off].max()) if off.any() else 0.0, "m")
            zero = (b32 == 0).all(axis=2)
            assert np.array_equal(got32[zero].view(np.uint32), b32[zero].view(np.uint32))
    # some motion really happened (the test is not comparing two copies of the input)
    assert np.abs(c.deskew_scans(batch, Q.lidar(), motions, 1.0) - batch).max() > 0.1


def rodrigues(axis, angle):
    """rotation matrices about a unit axis by (n,) angles — built without quaternions"""
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0.0]])
    return np.eye(3)[None] + np.sin(angle)[:, None, None] * K[None] + (1 - np.cos(angle))[:, None, None] * (K @ K)[None]


@pytest.mark.parametrize("flip", [False, True])
def test_convention_against_synthesised_measurements(flip):
    """Fixed world points, one per (line, column) of a 16 x 256 scan, seen by a sensor that moves 1.2 m and turns 3 degrees
    during the sweep: the measurements p_c = T(tau_c)^-1 P_w are synthesised in numpy (axis-angle rotations, no slerp), so
    a transposed rotation or a reversed time axis in the kernel cannot hide behind a restated formula. deskew(rho = 1) must
    give T(1)^-1 P_w, deskew(rho = 0) P_w itself, deskew(rho = 0.25) T(0.25)^-1 P_w."""
    h, w = 16, 256
    c = ctx()
    lidar = capi.LidarParams(h, w, 1.0, 120.0)
    rng = np.random.default_rng(77)
    axis = np.array([0.2, -0.1, 1.0])
    axis /= np.linalg.norm(axis)
    theta = np.radians(3.0)
    t = np.array([1.2, 0.1, -0.05])
    t *= 1.2 / np.linalg.norm(t)
    d = rng.normal(size=(h, w, 3))
    P_w = d / np.linalg.norm(d, axis=2, keepdims=True) * rng.uniform(5.0, 40.0, (h, w, 1))
    tau = np.arange(w) / w
    R = rodrigues(axis, tau * theta)                                          # R(tau_c): (w, 3, 3)
    meas = np.einsum("cji,lcj->lci", R, P_w - (tau[:, None] * t[None, :])[None])   # R^T (P_w - tau t)
    motion = np.concatenate([axis * np.sin(theta / 2), [np.cos(theta / 2)], t])
    if flip:
        motion[:4] = -motion[:4]
    flat = np.ascontiguousarray(meas.reshape(-1, 3))
    for rho in (1.0, 0.0, 0.25):
        Rr = rodrigues(axis, np.array([rho * theta]))[0]
        want = (P_w.reshape(-1, 3) - rho * t) @ Rr  # rows: R(rho)^T (P_w - rho t)
        got = c.deskew_scans(flat, lidar, motion[None], rho)
        check_points(got, want, flat, t, ("convention", rho, flip))
    assert np.abs(flat - P_w.reshape(-1, 3)).max() > 0.5  # (the sweep's motion is far above the bound)


def test_deskewed_scan_feeds_extraction(oracle):
    """a de-skewed canyon scan is a scan: extract_features on it equals the oracle's extraction of the downloaded array
    (no-return beams still zero and still refused by the range check)"""
    c = ctx()
    scans, motions = sequence_motions()
    for rho in (1.0, 0.0):
        out = c.deskew_scans(scans[2], Q.lidar(), motions[1], rho)
        assert np.array_equal((out == 0).all(axis=1), (scans[2] == 0).all(axis=1))
        e, p = c.extract_features(out, Q.lidar())
        oe, op = oracle.extract_features(out, H, W, 1.0, 120.0)
        assert len(oe) > 100 and len(op) > 10000
        assert np.array_equal(e, oe) and np.array_equal(p, op), rho
    # straight from device memory into the batch extraction, float scans included
    s32 = np.ascontiguousarray(scans[1:3].astype(np.float32))
    out32 = c.deskew_scans(s32, Q.lidar(), motions[:2], 1.0)
    for s in range(2):
        e, p = c.extract_features(out32[s], Q.lidar())
        oe, op = oracle.extract_features(out32[s].astype(np.float64), H, W, 1.0, 120.0)
        assert np.array_equal(e, oe) and np.array_equal(p, op), s


def test_refusals():
    c = ctx()
    scan = Q.sequence(*Q.SEQUENCES[0])[0]
    for rho in (-0.01, 1.01, np.nan):
        with pytest.raises(capi.LoamxError) as e:
            c.deskew_scans(scan, Q.lidar(), IDENT, rho)
        assert e.value.status == capi.ERR_BAD_PARAM
    with pytest.raises(ValueError):
        c.deskew_scans(scan[:-1], Q.lidar(), IDENT)
    with pytest.raises(ValueError):
        c.deskew_scans(scan, Q.lidar(), np.tile(IDENT, (2, 1)))
