"""CPU-only: info_math.h — the row, the accumulation and the 6x6 eigen-solve of the registration information matrix
(loam_amd/csrc/info_kernels.hip; include/loamx.h: loamx_reg_information) — compiled with g++ (tests/hostcheck_info) against
a 40-digit mpmath evaluation of the documented formulas and against numpy.linalg. The GPU tests (test_gpu_information*.py)
build their model of a record from the same g++ build."""
import ctypes as C
import os
import subprocess

import mpmath as mp
import numpy as np
import pytest

import info_common as I
from loam_amd import capi

mp.mp.dps = 40
# Worst error of a row entry relative to |v| |g| + |g| over the 4 000 records of test_row_accuracy_against_mpmath, as measured
# with this g++ build: 8.62e-12, at an edge point 1.19e-6 m from a line 0.2 m long — c = (v - a) x (v - b) is a
# difference of products of ~0.1 m vectors that cancels to ~2e-7 m^2. The test asserts 8x that figure.
ROW_ERROR_MEASURED = 8.62e-12


def mpv(a):
    return mp.matrix([mp.mpf(float(x)) for x in a])


def cross(a, b):
    return mp.matrix([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def norm(a):
    return mp.sqrt(dot(a, a))


def residual_mp(kind, v, prim):
    """r and g of the documented formulas in 40 digits"""
    if kind:
        n, d = mpv(prim[:3]), mp.mpf(float(prim[3]))
        s = dot(n, v) - d
        return abs(s), (n if s >= 0 else -n)
    a, b = mpv(prim[:3]), mpv(prim[3:6])
    c = cross(v - a, v - b)
    ab = a - b
    return norm(c) / norm(ab), cross(ab, c) / (norm(c) * norm(ab))


def row_mp(kind, v, prim):
    v = mpv(v)
    r, g = residual_mp(kind, v, prim)
    return list(cross(v, g)) + list(g), r, norm(v) * norm(g) + norm(g)


def random_records(rng, n):
    """planes and lines in general position with coordinates up to 120 m, the point 1e-6 .. 5 m from the primitive
    (log-uniform), a and b 0.2 m apart around the foot point as fit_line makes them"""
    kind, v, prim = np.zeros(2 * n, dtype=np.uint8), np.zeros((2 * n, 3)), np.zeros((2 * n, 6))
    for i in range(2 * n):
        foot = rng.uniform(-120, 120, 3) * np.array([1, 1, 0.1])
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        w = np.cross(u, rng.normal(size=3))
        w /= np.linalg.norm(w)
        dist = 10 ** rng.uniform(-6, np.log10(5.0))
        if i % 2:  # plane with normal u through foot; the point off it by +-dist, anywhere within 2 m on the plane
            kind[i] = 1
            v[i] = foot + rng.choice([-1, 1]) * dist * u + rng.uniform(-2, 2) * w
            prim[i, :3], prim[i, 3] = u, float(np.dot(u, foot))
        else:  # line through foot along u
            centre = foot + rng.uniform(-0.3, 0.3) * u
            v[i] = foot + dist * w
            prim[i, :3], prim[i, 3:] = centre + 0.1 * u, centre - 0.1 * u
    return kind, v, prim


def test_row_accuracy_against_mpmath():
    kind, v, prim = random_records(np.random.default_rng(41), 2000)
    J, r, finite, _ = I.rows(kind, v, prim, scaled=False)
    assert finite.all()
    worst, worst_r, at = 0.0, 0.0, -1
    for i in range(len(kind)):
        Jm, rm, scale = row_mp(int(kind[i]), v[i], prim[i])
        e = max(abs(mp.mpf(float(J[i, j])) - Jm[j]) for j in range(6)) / scale
        if e > worst:
            worst, at = float(e), i
        worst_r = max(worst_r, float(abs(mp.mpf(float(r[i])) - rm) / (rm + mp.mpf(2) ** -52 * 120)))
    d = float(residual_mp(int(kind[at]), mpv(v[at]), prim[at])[0])
    print(f"worst row error relative to |v||g| + |g|: {worst:.3g} (record {at}, kind {int(kind[at])}, {d:.3g} m from its primitive); worst residual error {worst_r:.3g}")
    assert worst <= 8 * ROW_ERROR_MEASURED
    planes = kind == 1  # (a plane row is a sign and a cross product: a few units in the last place)
    worst_plane = max(float(max(abs(mp.mpf(float(J[i, j])) - row_mp(1, v[i], prim[i])[0][j]) for j in range(6)) / row_mp(1, v[i], prim[i])[2])
                      for i in np.flatnonzero(planes)[:300])
    assert worst_plane <= 8 * 2.0 ** -52, worst_plane


def rot_mp(w):
    """Exp of a rotation vector (Rodrigues) in 40 digits"""
    th = norm(w)
    K = mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th == 0:
        return mp.eye(3)
    return mp.eye(3) + mp.sin(th) / th * K + (1 - mp.cos(th)) / th ** 2 * (K * K)


def test_row_is_the_derivative_for_the_left_perturbation_rotation_first():
    """J = d r(Exp(delta) o T . p) / d delta at 0 with Exp([omega, t]) v = R(omega) v + t: central differences in mpmath"""
    rng = np.random.default_rng(42)
    kind, v, prim = random_records(rng, 30)
    keep = np.array([float(residual_mp(int(kind[i]), mpv(v[i]), prim[i])[0]) > 1e-3 for i in range(len(kind))])
    kind, v, prim = kind[keep], v[keep], prim[keep]
    assert (kind == 0).sum() >= 10 and (kind == 1).sum() >= 10
    J, r, finite, _ = I.rows(kind, v, prim, scaled=False)
    h = mp.mpf(10) ** -12
    worst = 0.0
    for i in range(len(kind)):
        vi = mpv(v[i])
        _, _, scale = row_mp(int(kind[i]), v[i], prim[i])
        for j in range(6):
            def r_at(step):
                d = mp.matrix([0] * 6)
                d[j] = step
                moved = rot_mp(d[:3]) * vi + mp.matrix(list(d[3:]))
                return residual_mp(int(kind[i]), moved, prim[i])[0]
            fd = (r_at(h) - r_at(-h)) / (2 * h)
            worst = max(worst, float(abs(mp.mpf(float(J[i, j])) - fd) / scale))
    print(f"worst |J - central difference| relative to |v||g| + |g|: {worst:.3g}")
    assert worst <= 1e-9
    # the other conventions are far away: a right perturbation (axes of the SOURCE frame) or translation first would move
    # the rotational block by |t x g| ~ the size of the entries themselves — asserted by the magnitude of the block
    assert np.abs(J[:, :3]).max() > 1.0


def test_huber_scaling_on_both_sides_of_one_and_dropped_rows():
    n = [0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    below, at, above = np.nextafter(1.0, 0.0), 1.0, np.nextafter(1.0, 2.0)
    kind = np.array([1, 1, 1, 1, 0, 0, 0, 0], dtype=np.uint8)
    v = np.array([[1, 2, below], [1, 2, at], [1, 2, above], [1, 2, -4.0],  # planes z = 0: r = |z|
                  [0.5, 0.0, 2.0], [0.5, 0.0, 0.25],                       # edges along x through the origin: r = |z|
                  [0.3, 0.0, 0.0],                                         # on the line: |c| = 0
                  [0.3, 1.0, 0.0]])                                        # a = b
    prim = np.array([n, n, n, n, [0.1, 0, 0, -0.1, 0, 0], [0.1, 0, 0, -0.1, 0, 0], [0.1, 0, 0, -0.1, 0, 0], [0.1, 0, 0, 0.1, 0, 0]])
    Ju, ru, fu, _ = I.rows(kind, v, prim, scaled=False)
    Js, rs, fs, hub = I.rows(kind, v, prim, scaled=True)
    assert fu.tolist() == [True] * 6 + [False, False] and fs.tolist() == fu.tolist()
    assert hub.tolist() == [False, False, above * above > 1.0, True, True, False, False, False]
    assert above * above > 1.0 and not (below * below > 1.0)
    for i in (0, 1, 5):  # r^2 <= 1: untouched, bit for bit
        assert np.array_equal(Js[i], Ju[i]) and rs[i] == ru[i]
    for i in (2, 3, 4):  # r^2 > 1: scaled by sqrt(1 / r) as residual_accumulate does (sqrt(1 / sqrt(r^2)))
        sc = np.sqrt(1.0 / np.sqrt(ru[i] * ru[i]))
        assert np.array_equal(Js[i], Ju[i] * sc) and rs[i] == ru[i] * sc
    assert np.allclose(ru[:6], [below, 1.0, above, 4.0, 2.0, 0.25], rtol=1e-15)
    assert np.allclose(Ju[3], [-2.0, 1.0, 0.0, 0.0, 0.0, -1.0])  # g = -n below the plane, J = [v x g, g]
    sums, cnt = I.accumulate(kind, v, prim)
    assert cnt.tolist() == [2, 4, 3, 2]  # n_edge, n_plane, n_huber, n_dropped
    m = I.model(kind, v, prim)
    assert (m["n_edge"], m["n_plane"], m["n_huber"], m["n_dropped"]) == (2, 4, 3, 2)
    assert np.all(np.isfinite(sums)) and np.all(np.abs(sums - m["want"]) <= m["n"] * I.EPS * m["mag"])
    assert sums[27] == pytest.approx(below ** 2 + 1 + above + 4 + 2 + 0.0625, rel=1e-14)  # scaled r^2 = r beyond the threshold


def corridor_matrix():
    """the rank-5 matrix of the exact corridor: rows built from the lattice itself (walls x = +-2 with normals +-e_x, floor and
    ceiling z = +-1.5, junction lines along y), so that nothing constrains t_y"""
    se, sp, _, _ = I.corridor()
    kind = np.concatenate([np.zeros(len(se), dtype=np.uint8), np.ones(len(sp), dtype=np.uint8)])
    prim = np.zeros((len(kind), 6))
    for i, p in enumerate(se):
        foot = np.array([2.0 * np.sign(p[0]), round(p[1] * 4) / 4, 1.5 * np.sign(p[2])])
        prim[i, :3], prim[i, 3:] = foot + [0, 0.1, 0], foot - [0, 0.1, 0]
    for i, p in enumerate(sp, start=len(se)):
        wall = abs(abs(p[0]) - 2.0) < 0.1
        prim[i, :4] = [np.sign(p[0]), 0, 0, 2.0] if wall else [0, 0, np.sign(p[2]), 1.5]
    sums, cnt = I.accumulate(kind, np.concatenate([se, sp]), prim)
    assert cnt.tolist() == [196, 1568, 0, 0]
    return I.mirror(sums[:21])


def test_eig6_against_numpy_eigh():
    rng = np.random.default_rng(43)
    cases = []
    for cond in (1.0, 1e3, 1e6, 1e9, 1e12):
        for scale in (1.0, 1e4):
            for _ in range(6):
                Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
                lam = scale * cond ** -rng.uniform(0, 1, 6)
                lam[0], lam[5] = scale / cond, scale
                M = (Q * lam) @ Q.T
                cases.append((f"spd cond {cond:g} scale {scale:g}", (M + M.T) / 2))
    cases.append(("zero", np.zeros((6, 6))))
    cases.append(("diagonal descending", np.diag([6.0, 5, 4, 3, 2, 1])))
    cases.append(("diagonal mixed", np.diag([3.0, 1e-9, 7e5, 0.0, 2.0, 2.0])))
    cases.append(("identity", np.eye(6)))
    Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
    cases.append(("repeated 1 1 1 5 5 9", (Q * np.array([1.0, 1, 1, 5, 5, 9])) @ Q.T))
    cases.append(("repeated 2 x3 + 0 x3", (Q * np.array([2.0, 2, 2, 0, 0, 0])) @ Q.T))
    cases.append(("corridor rank 5", corridor_matrix()))
    most = 0
    for name, M in cases:
        M = (M + M.T) / 2
        lam, vec, sweeps = I.eig6(M)
        most = max(most, sweeps)
        mu = I.check_eigenpairs(M, lam, vec, name)
        assert np.abs(lam - mu).max() <= 64 * I.EPS * max(np.linalg.norm(M), 1e-300), name  # (Weyl: both are backward stable)
    assert most < I.lib().hostcheck_info_sweep_cap() // 2, most
    lam, vec, sweeps = I.eig6(np.zeros((6, 6)))
    assert sweeps == 0 and np.array_equal(lam, np.zeros(6)) and np.array_equal(vec, np.eye(6))  # a pair without a row
    lam, vec, _ = I.eig6(np.diag([6.0, 5, 4, 3, 2, 1]))
    assert np.array_equal(lam, [1, 2, 3, 4, 5, 6]) and np.array_equal(vec, np.eye(6)[::-1])
    lam, vec, _ = I.eig6(corridor_matrix())
    assert lam[0] == 0.0 and np.array_equal(vec[0], [0, 0, 0, 0, 1, 0]) and lam[1] > 100  # t_y, exactly
    # only the upper triangle is read
    M = cases[7][1].copy()
    lam0, vec0, _ = I.eig6(M)
    M[np.tril_indices(6, -1)] = 123.0
    lam1, vec1, _ = I.eig6(M)
    assert np.array_equal(lam0, lam1) and np.array_equal(vec0, vec1)
    # sign rule on a tie: (1, 1) / sqrt 2 and (1, -1) / sqrt 2 in the 0-1 plane -> the component of LOWEST index is positive
    T = np.diag([0.0, 0, 3, 4, 5, 6])
    T[0, 0] = T[1, 1] = 2.0
    T[0, 1] = T[1, 0] = 1.0
    lam, vec, _ = I.eig6(T)
    assert lam[:2].tolist() == [1.0, 3.0] and vec[0, 0] > 0 > vec[0, 1] and vec[1, 0] > 0 and vec[1, 1] > 0


def info_of(H, weighted_sq_error, n_edge, n_plane):
    lam, vec, _ = I.eig6(H)
    rec = np.zeros(1, dtype=capi.INFORMATION_DTYPE)
    rec["information"], rec["eigenvalues"], rec["eigenvectors"] = H, lam, vec
    rec["weighted_sq_error"], rec["n_edge"], rec["n_plane"] = weighted_sq_error, n_edge, n_plane
    return capi.RegInformation.from_record(rec[0])


def test_covariance_and_degenerate_directions_against_numpy_pinv():
    assert C.sizeof(capi.RegInformation) == 696 == capi.INFORMATION_DTYPE.itemsize
    rng = np.random.default_rng(44)
    A = rng.normal(size=(40, 6)) * np.array([30, 30, 30, 1, 1, 1])
    H = A.T @ A
    info = info_of(H, 0.37, 10, 30)
    assert np.array_equal(info.information, H) and info.information.shape == (6, 6) and info.eigenvectors.shape == (6, 6)
    want = I.covariance_numpy(H, 0.37, 40)
    assert np.abs(info.covariance() - want).max() <= 1e-10 * np.abs(want).max()
    assert len(info.degenerate_directions(1e-3)) == 0
    assert np.array_equal(info.degenerate_directions(info.eigenvalues[2] * 1.0001), info.eigenvectors[:3])
    # rank 5: the corridor. The unobservable direction takes no part in the covariance and is what degenerate_directions returns
    Hc = corridor_matrix()
    info = info_of(Hc, 8.0, 196, 1568)
    want = I.covariance_numpy(Hc, 8.0, 196 + 1568)
    cov = info.covariance()
    assert np.abs(cov - want).max() <= 1e-10 * np.abs(want).max() and np.all(cov[4] == 0) and np.all(cov[:, 4] == 0)
    deg = info.degenerate_directions(100.0)
    assert deg.shape == (1, 6) and np.array_equal(deg[0], [0, 0, 0, 0, 1, 0])
    # a threshold that keeps fewer directions
    loose = info_of(H, 0.37, 10, 30).covariance(rel_threshold=0.5)
    lam, vec = np.linalg.eigh(H)
    keep = lam > 0.5 * lam[-1]
    want = 0.37 / 34 * (vec[:, keep] / lam[keep]) @ vec[:, keep].T
    assert np.abs(loose - want).max() <= 1e-10 * np.abs(want).max()
    with pytest.raises(ValueError):
        info_of(H, 0.37, 2, 4).covariance()  # six rows determine no variance
    with pytest.raises(ValueError):
        info_of(np.zeros((6, 6)), 0.0, 0, 0).covariance()


def test_the_same_functions_are_clean_under_asan_and_ubsan_in_a_stand_alone_program():
    subprocess.check_call(["make", "-s", "-C", I.DIR, "san"])
    out = subprocess.run([os.path.join(I.DIR, "hostcheck_info_san")], capture_output=True, text=True, timeout=300)
    text = out.stdout + out.stderr
    assert out.returncode == 0 and "hostcheck_info ok" in out.stdout, text[-3000:]
    assert "runtime error" not in text and "AddressSanitizer" not in text, text[-3000:]
