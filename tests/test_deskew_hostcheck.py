"""CPU-only: deskew_math.h — what deskew_kernel (loam_amd/csrc/sequence_kernels.hip) computes once per column (motion load,
slerp, m = R(rho)^T R(tau), d = R(rho)^T (tau - rho) t) and once per point — compiled with g++ (tests/hostcheck_deskew) against
40-digit mpmath arithmetic. The reference has no quaternion slerp in it: the motion quaternion is normalised, put on the short
arc (negated iff w < 0; w = -0.0 is not below zero), read as the rotation by theta = 2 atan2(|v|, w) about v / |v|, and R(tau),
R(rho) are the axis-angle (Rodrigues) matrices of tau theta and rho theta.

The measure of a column: e = (|m - m_ref|_F + |d - d_ref|) / (2 + |t|), the error of a point with |p| = 1 over what bound() of
tests/test_gpu_deskew.py allows it per 1e-12 m (1e-12 (1 + |p| + |t|)); e <= 1e-12 is that allowance. Measured with g++ -O2
-ffp-contract=off and glibc on x86-64 over every case below: worst e = 5.7e-16 (MEASURED_WORST; a 1e-150-scaled quaternion at
tau = 0, rho = 1; random motions 5.5e-16, half turns 4.5e-16, the small-angle seam 1.2e-16). Asserted: 8 x that, libm's sin / cos / atan2
differing between machines by a few ulp — and never looser than 1e-12."""
import ctypes as C
import functools
import os
import subprocess

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "hostcheck_deskew")
MEASURED_WORST = 5.7e-16
FACTOR = 8
LIMIT = min(FACTOR * MEASURED_WORST, 1e-12)
# m is a product of two rotation matrices of quaternions (sin(h) v / |v|, cos(h)) whose norms are 1 within ~4 roundings; a matrix of
# a quaternion of norm 1 + e is orthogonal within ~4 e: 2 x 4 x 4 x 1.1e-16 plus the ~6 roundings of the 3 x 3 product, ~5x margin
# (measured worst: 3.2e-15)
ORTHO_LIMIT = 2e-14
_lib = None
mp = mpmath.mp.clone()
mp.dps = 40


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", DIR])
        _lib = C.CDLL(os.path.join(DIR, "libhostcheck_deskew.so"))
    return _lib


def header_columns(motions, tau, rho):
    """(n, 7), (n,), (n,) -> q (n, 4) as deskew_load_motion hands it on, m (n, 3, 3), d (n, 3)"""
    motions = np.ascontiguousarray(motions, dtype=np.float64).reshape(-1, 7)
    n = len(motions)
    tau, rho = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (n,))) for v in (tau, rho))
    q, col = np.zeros((n, 4)), np.zeros((n, 12))
    dp = C.POINTER(C.c_double)
    lib().hostcheck_deskew_columns(motions.ctypes.data_as(dp), tau.ctypes.data_as(dp), rho.ctypes.data_as(dp), C.c_uint64(n),
                                   q.ctypes.data_as(dp), col.ctypes.data_as(dp))
    return q, col[:, :9].reshape(n, 3, 3).copy(), col[:, 9:].copy()


def header_points(m, d, pts):
    col = np.ascontiguousarray(np.concatenate([np.asarray(m, dtype=np.float64).reshape(9), np.asarray(d, dtype=np.float64).reshape(3)]))
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    out, moved = np.zeros_like(pts), np.zeros(len(pts), dtype=np.uint8)
    dp = C.POINTER(C.c_double)
    lib().hostcheck_deskew_points(col.ctypes.data_as(dp), pts.ctypes.data_as(dp), C.c_uint64(len(pts)), out.ctypes.data_as(dp),
                                  moved.ctypes.data_as(C.POINTER(C.c_uint8)))
    return out, moved.astype(bool)


def rodrigues_mp(axis, angle):
    """rotation matrix about a unit axis — no quaternion in it"""
    K = mp.matrix([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return mp.eye(3) + mp.sin(angle) * K + (1 - mp.cos(angle)) * (K * K)


@functools.lru_cache(maxsize=None)
def axis_angle_mp(quat):
    """the double quaternion (a tuple, as given: any norm, either sign) -> (unit axis, theta in [0, pi]) at 40 digits"""
    x, y, z, w = (mp.mpf(float(v)) for v in quat)
    n = mp.sqrt(x * x + y * y + z * z + w * w)
    if float(quat[3]) < 0.0:  # the short arc; -0.0 is not below zero
        n = -n
    x, y, z, w = x / n, y / n, z / n, w / n
    vn = mp.sqrt(x * x + y * y + z * z)
    if vn == 0:
        return (mp.mpf(1), mp.mpf(0), mp.mpf(0)), mp.mpf(0)
    return (x / vn, y / vn, z / vn), 2 * mp.atan2(vn, w)


def reference_column(motion, tau, rho):
    """m_ref (3, 3), d_ref (3,) as mp matrices; tau and rho are the doubles the kernel holds"""
    axis, theta = axis_angle_mp(tuple(float(v) for v in motion[:4]))
    tau, rho = mp.mpf(float(tau)), mp.mpf(float(rho))
    Rr_T = rodrigues_mp(axis, rho * theta).T
    t = mp.matrix([mp.mpf(float(v)) for v in motion[4:]])
    return Rr_T * rodrigues_mp(axis, tau * theta), Rr_T * ((tau - rho) * t)


def column_error(motion, tau, rho, m, d):
    m_ref, d_ref = reference_column(motion, tau, rho)
    em = mp.sqrt(sum((mp.mpf(float(m[i, j])) - m_ref[i, j]) ** 2 for i in range(3) for j in range(3)))
    ed = mp.sqrt(sum((mp.mpf(float(d[i])) - d_ref[i]) ** 2 for i in range(3)))
    return float((em + ed) / (2 + mp.sqrt(sum(mp.mpf(float(v)) ** 2 for v in motion[4:]))))


def fractions(w):
    return [0.0, 1.0 / w, 0.5, (w - 1.0) / w, 1.0]  # ((w - 1) / w: the double c / W the kernel forms for the last column)


def unit_quats(rng, angles):
    axis = rng.normal(size=(len(angles), 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    return np.concatenate([axis * np.sin(angles / 2)[:, None], np.cos(angles / 2)[:, None]], axis=1)


def check(what, motions, tau, rho):
    """every column: orthogonal, and within LIMIT of the reference; returns the worst e"""
    motions = np.asarray(motions, dtype=np.float64).reshape(-1, 7)
    tau, rho = (np.broadcast_to(np.asarray(v, dtype=np.float64), (len(motions),)) for v in (tau, rho))
    _, m, d = header_columns(motions, tau, rho)
    ortho = np.linalg.norm(np.einsum("nij,nkj->nik", m, m) - np.eye(3), axis=(1, 2))
    assert np.isfinite(m).all() and np.isfinite(d).all(), what
    assert (ortho <= ORTHO_LIMIT).all(), (what, ortho.max())
    assert (np.linalg.det(m) > 0.5).all(), what
    e = np.array([column_error(motions[i], tau[i], rho[i], m[i], d[i]) for i in range(len(motions))])
    i = int(e.argmax())
    print(what, len(e), "columns: worst e", e[i], "(motion", motions[i].tolist(), "tau", tau[i], "rho", rho[i], ") limit", LIMIT,
          "; worst |m m^T - 1|", ortho.max())
    assert (e <= LIMIT).all(), (what, e[i], motions[i].tolist(), tau[i], rho[i])
    return e[i]


def grid(motions, w=1024):
    """every motion at every (tau, rho) of fractions(w)"""
    f = fractions(w)
    mo = np.repeat(np.asarray(motions, dtype=np.float64).reshape(-1, 7), len(f) * len(f), axis=0)
    tr = np.array([(a, b) for a in f for b in f] * (len(mo) // (len(f) * len(f))))
    return mo, tr[:, 0], tr[:, 1]


def test_random_motions_with_angles_from_1e_minus_15_to_pi():
    """400 motions, angle log-uniform in [1e-15, pi], t in uniform(-5, 5); each at three (tau, rho): one from the grid
    {0, 1/W, 0.5, 1 - 1/W, 1}^2, one (c / W, grid) for a random column, one (c / W, uniform)"""
    rng = np.random.default_rng(11)
    n = 400
    angles = np.exp(rng.uniform(np.log(1e-15), np.log(np.pi), n))
    angles[:4] = [1e-15, np.pi, np.nextafter(np.pi, 0), 2e-12]
    motions = np.concatenate([unit_quats(rng, angles), rng.uniform(-5, 5, (n, 3))], axis=1)
    worst = 0.0
    for k, w in enumerate((1024, 1800, 37)):
        f = np.array(fractions(w))
        col = rng.integers(0, w, n) / float(w)
        tau = (f[rng.integers(0, 5, n)], col, col)[k]
        rho = (f[rng.integers(0, 5, n)], f[rng.integers(0, 5, n)], rng.uniform(0, 1, n))[k]
        worst = max(worst, check("random, W = %d" % w, motions, tau, rho))
    assert worst > 0.0  # (the comparison is not between two copies of one computation)


def test_the_seam_of_the_small_angle_branch():
    """|v| in {0, 1e-14, 9.99e-13, 1e-12, 1.01e-12, 1e-10} beside w = 1 (the norm is then 1 in double and |v| reaches
    deskew_slerp as given): along an axis, along (0, -0.6, 0.8), along a random direction; as given and scaled by -3"""
    rng = np.random.default_rng(12)
    motions = []
    for vn in (0.0, 1e-14, 9.99e-13, 1e-12, 1.01e-12, 1e-10):
        r = rng.normal(size=3)
        for direction in ([1.0, 0, 0], [0, -0.6, 0.8], r / np.linalg.norm(r)):
            for scale in (1.0, -3.0):
                motions.append(np.concatenate([scale * np.append(vn * np.asarray(direction), 1.0), rng.uniform(-5, 5, 3)]))
    q, _, _ = header_columns(motions, 0.0, 0.0)
    vn = np.linalg.norm(q[:, :3], axis=1)
    assert (vn < 1e-12).sum() >= 12 and (vn >= 1e-12).sum() >= 12, "the cases no longer lie on both sides of the seam"
    check("seam", *grid(motions))


def test_half_turns_and_the_sign_rule_at_w_zero():
    """w in {+0.0, -0.0, +-1e-300, +-1e-9} beside a unit v: the half turn. The header negates the quaternion iff w < 0, so w =
    -0.0 is NOT negated: it turns about +v like w = +0.0 (bit for bit), w = -1e-300 about -v. Half way (tau = 0.5) the two
    differ by a half turn, so the agreement with the reference, which applies the same rule, pins which one is taken."""
    v = np.array([0.6, 0.0, -0.8])
    t = np.array([1.5, -2.0, 0.25])
    ws = [0.0, -0.0, 1e-300, -1e-300, 1e-9, -1e-9]
    motions = [np.concatenate([v, [w], t]) for w in ws] + [np.concatenate([-3.0 * v, [-3.0 * w], t]) for w in ws]
    check("half turns", *grid(motions))
    q, m, d = header_columns(motions[:6], 0.5, 0.0)
    assert np.array_equal(q[0, :3], v) and np.array_equal(q[1, :3], v) and q[0, 3] == 0 and q[1, 3] == 0  # -0.0: as given
    assert np.array_equal(m[0], m[1]) and np.array_equal(d[0], d[1])
    assert np.array_equal(q[3, :3], -v) and q[3, 3] == 1e-300 and np.array_equal(q[2, :3], v)
    # a quarter turn about +v against one about -v: transposes of each other, far apart
    assert np.abs(m[2] - m[3].T).max() < 1e-15 and np.abs(m[2] - m[3]).max() > 1.0
    assert np.abs(m[0] - m[2]).max() < 1e-15 and np.abs(m[4] - m[5].T).max() < 1e-8


def test_quaternions_of_any_norm_within_the_documented_range():
    """scaled by {1e-3, -3, 1e3, 1e-150, 1e150} (include/loamx.h: the norm must lie in [1e-150, 1e150])"""
    rng = np.random.default_rng(13)
    base = unit_quats(rng, np.array([1e-13, 1e-3, 0.3, 2.0, np.pi - 1e-9]))
    motions = [np.concatenate([s * q, rng.uniform(-5, 5, 3)]) for q in base for s in (1e-3, -3.0, 1e3, 1e-150, 1e150)]
    check("scaled", *grid(motions, 1800))


def test_identity_motions_give_the_identity_matrix_and_the_plain_offset_exactly():
    f = fractions(1024)
    for quat in ([0, 0, 0, 1.0], [0, 0, 0, -2.5], [0, 0, 0, 1e-150], [-0.0, 0.0, -0.0, 1e150]):
        for t in ([0.0, 0.0, 0.0], [1.5, -2.0, 0.25]):
            mo, tau, rho = grid([np.concatenate([quat, t])])
            _, m, d = header_columns(mo, tau, rho)
            assert (m == np.eye(3)).all(), quat
            assert (d == (tau - rho)[:, None] * np.asarray(t)[None, :]).all(), (quat, t)  # (zero for t = 0)
    # and then a finite, non-zero point comes back bit for bit
    pts = np.random.default_rng(14).uniform(-100, 100, (1000, 3))
    _, m, d = header_columns([[0, 0, 0, -2.5, 0, 0, 0]], f[3], f[2])
    out, moved = header_points(m[0], d[0], pts)
    assert moved.all() and np.array_equal(out.view(np.uint64), pts.view(np.uint64))


def test_points_zero_and_non_finite_are_left_alone_the_rest_is_m_p_plus_d():
    rng = np.random.default_rng(15)
    motion = np.concatenate([unit_quats(rng, np.array([2.0]))[0] * -3.0, [1.5, -2.0, 0.25]])
    _, m, d = header_columns([motion], 0.25, 1.0)
    pts = rng.uniform(-100, 100, (2000, 3))
    special = np.array([[0.0, 0.0, 0.0], [-0.0, 0.0, -0.0], [np.nan, 1, 2], [3, -np.inf, 2], [1, 2, np.inf], [np.nan, np.nan, np.nan]])
    alive = np.array([[0.0, 0.0, 1e-300], [0.0, -0.0, 5.0], [1e300, 0, 0]])
    out, moved = header_points(m[0], d[0], np.concatenate([special, alive, pts]))
    assert not moved[:6].any() and moved[6:].all()
    assert np.array_equal(out[:6].view(np.uint64), special.view(np.uint64))
    m_ref, d_ref = reference_column(motion, 0.25, 1.0)
    tn = float(np.linalg.norm(motion[4:]))
    worst = 0.0
    for p, o in zip(pts[:300], out[9:309]):
        want = m_ref * mp.matrix([mp.mpf(float(v)) for v in p]) + d_ref
        err = float(mp.sqrt(sum((mp.mpf(float(o[i])) - want[i]) ** 2 for i in range(3))))
        worst = max(worst, err / (1e-12 * (1.0 + float(np.linalg.norm(p)) + tn)))
    print("points against mpmath: worst error / bound()", worst)
    assert worst <= 1.0


def test_a_quaternion_without_direction_gives_nan_pinned():
    """include/loamx.h: the norm of the motion quaternion must lie in [1e-150, 1e150]. The zero quaternion, and one whose squares
    underflow to 0, have no direction: every number of the column is NaN and so is every finite non-zero point of that scan,
    silently (zero and non-finite points are still copied). Pinned so that a change of this behaviour is a decision."""
    for quat in ([0.0, 0.0, 0.0, 0.0], [0.0, -0.0, 0.0, -0.0], [3e-170, 1e-170, 2e-170, 9e-170], [0, 0, 0, 1e-170]):
        mo, tau, rho = grid([np.concatenate([quat, [1.5, -2.0, 0.25]])])
        _, m, d = header_columns(mo, tau, rho)
        assert np.isnan(m).all() and np.isnan(d).all(), quat
        out, moved = header_points(m[0], d[0], [[1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [np.nan, 1.0, 2.0]])
        assert moved.tolist() == [True, False, False] and np.isnan(out[0]).all() and (out[1] == 0).all() and out[2, 1] == 1.0, quat


def test_the_same_functions_are_clean_under_asan_and_ubsan_in_a_stand_alone_program():
    subprocess.check_call(["make", "-s", "-C", DIR, "san"])
    out = subprocess.run([os.path.join(DIR, "hostcheck_deskew_san")], capture_output=True, text=True, timeout=300)
    text = out.stdout + out.stderr
    assert out.returncode == 0 and "hostcheck_deskew ok" in out.stdout, text[-3000:]
    assert "runtime error" not in text and "AddressSanitizer" not in text, text[-3000:]
