"""Shared by the registration-information tests (CPU and GPU): the g++ build of loam_amd/csrc/info_math.h
(tests/hostcheck_info), the exact-sum model of a record built from an association dump, the eigenpair rule and the
corridor lattice."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "hostcheck_info")
EPS = 2.0 ** -52
_lib = None
_dp, _u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
# upper triangle in the order of InfoAcc::s (row-major)
TRI = [(i, j) for i in range(6) for j in range(i, 6)]


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", DIR])
        _lib = C.CDLL(os.path.join(DIR, "libhostcheck_info.so"))
    return _lib


def rows(kind, v, prim, scaled=True):
    """info_row (+ info_huber when scaled) of every record: J (n, 6), r (n,), finite (n,) bool, huber (n,) bool"""
    kind = np.ascontiguousarray(kind, dtype=np.uint8)
    v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 3)
    prim = np.ascontiguousarray(prim, dtype=np.float64).reshape(-1, 6)
    n = len(kind)
    assert len(v) == n and len(prim) == n
    J, r, flags = np.zeros((n, 6)), np.zeros(n), np.zeros(n, dtype=np.uint8)
    lib().hostcheck_info_rows(C.c_uint64(n), kind.ctypes.data_as(_u8p), v.ctypes.data_as(_dp), prim.ctypes.data_as(_dp),
                              C.c_int(1 if scaled else 0), J.ctypes.data_as(_dp), r.ctypes.data_as(_dp), flags.ctypes.data_as(_u8p))
    return J, r, (flags & 1).astype(bool), (flags & 2).astype(bool)


def accumulate(kind, v, prim):
    """the records in order through info_accumulate: sums (28,), counters (4,)"""
    kind = np.ascontiguousarray(kind, dtype=np.uint8)
    v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 3)
    prim = np.ascontiguousarray(prim, dtype=np.float64).reshape(-1, 6)
    sums, cnt = np.zeros(28), np.zeros(4, dtype=np.uint32)
    lib().hostcheck_info_accumulate(C.c_uint64(len(kind)), kind.ctypes.data_as(_u8p), v.ctypes.data_as(_dp), prim.ctypes.data_as(_dp),
                                    sums.ctypes.data_as(_dp), cnt.ctypes.data_as(C.POINTER(C.c_uint32)))
    return sums, cnt


def mirror(tri):
    tri, H = np.ascontiguousarray(tri, dtype=np.float64), np.zeros((6, 6))
    lib().hostcheck_info_mirror(tri.ctypes.data_as(_dp), H.ctypes.data_as(_dp))
    return H


def eig6(H):
    """info_eig6: eigenvalues (6,), eigenvectors (6, 6) rows, sweeps"""
    H = np.ascontiguousarray(H, dtype=np.float64).reshape(6, 6)
    lam, vec = np.zeros(6), np.zeros((6, 6))
    sweeps = lib().hostcheck_info_eig6(H.ctypes.data_as(_dp), lam.ctypes.data_as(_dp), vec.ctypes.data_as(_dp))
    return lam, vec, sweeps


def records_of_dump(dump):
    """the VALID associations of a Context.associate dump as (kind, v, prim6): the bytes information_kernel reads"""
    e, p = dump["edge"], dump["plane"]
    ve, vp = e["valid"], p["valid"]
    kind = np.concatenate([np.zeros(int(ve.sum()), dtype=np.uint8), np.ones(int(vp.sum()), dtype=np.uint8)])
    v = np.concatenate([e["moved"][ve], p["moved"][vp]])
    prim = np.concatenate([e["prim"][ve], np.concatenate([p["prim"][vp], np.zeros((int(vp.sum()), 2))], axis=1)])
    return kind, v, prim


def model(kind, v, prim):
    """The record's sums from the scaled rows of info_math.h, every sum taken exactly (math.fsum): want (28,), the sums of the
    terms' magnitudes abs (28,), the four counters and the number of rows."""
    J, r, finite, huber = rows(kind, v, prim, scaled=True)
    kind = np.asarray(kind)
    Jf, rf = J[finite], r[finite]
    terms = [Jf[:, i] * Jf[:, j] for i, j in TRI] + [Jf[:, j] * rf for j in range(6)] + [rf * rf]
    want = np.array([math.fsum(t) for t in terms])
    mag = np.array([math.fsum(np.abs(t)) for t in terms])
    counters = dict(n_edge=int((finite & (kind == 0)).sum()), n_plane=int((finite & (kind == 1)).sum()),
                    n_huber=int((finite & huber).sum()), n_dropped=int((~finite).sum()))
    return dict(want=want, mag=mag, n=int(finite.sum()), **counters)


def record_sums(info):
    """(28,) sums of a record in the order of the model: upper triangle, gradient, weighted_sq_error"""
    H = np.asarray(info.information).reshape(6, 6)
    return np.concatenate([[H[i, j] for i, j in TRI], np.asarray(info.gradient), [float(info.weighted_sq_error)]])


def check_against_model(info, m, what=""):
    """The record may differ from the model by its summation order only: |got - want| <= n 2^-52 sum |term| (the bound of
    recursive summation in any order), entry by entry; equal counters; a bitwise symmetric matrix."""
    got = record_sums(info)
    bound = m["n"] * EPS * m["mag"]
    worst = np.max(np.abs(got - m["want"]) / np.where(bound > 0, bound, 1.0))
    print(f"{what}: rows {m['n_edge']} + {m['n_plane']}, huber {m['n_huber']}, dropped {m['n_dropped']}, worst |got - want| / bound = {worst:.3g}")
    assert (int(info.n_edge), int(info.n_plane), int(info.n_huber), int(info.n_dropped)) == (m["n_edge"], m["n_plane"], m["n_huber"], m["n_dropped"]), what
    assert np.all(np.isfinite(got)), what
    assert np.all(np.abs(got - m["want"]) <= bound), (what, got - m["want"], bound)
    H = np.asarray(info.information).reshape(6, 6)
    assert H.tobytes() == np.ascontiguousarray(H.T).tobytes(), what


def _inf_norm(M):
    return float(np.max(np.sum(np.abs(M), axis=1))) if M.ndim == 2 else float(np.max(np.abs(M)))


def eig_residuals(H, lam, vec):
    """(||V V^T - I||inf, max_i ||H v_i - lam_i v_i||inf) for eigenvectors in the ROWS of vec"""
    H, lam, vec = np.asarray(H, dtype=np.float64).reshape(6, 6), np.asarray(lam), np.asarray(vec).reshape(6, 6)
    return _inf_norm(vec @ vec.T - np.eye(6)), max(_inf_norm(H @ vec[i] - lam[i] * vec[i]) for i in range(6))


def check_eigenpairs(H, lam, vec, what=""):
    """Ascending eigenvalues, the sign rule, and both residuals at most 16 x max(numpy.linalg.eigh's own residual on this
    matrix, 8 * 2^-52 * scale): scale = ||H||_F for the eigen-residual; for the orthogonality, which has no unit, the smaller
    of 1 and ||H||_F."""
    H, lam, vec = np.asarray(H, dtype=np.float64).reshape(6, 6), np.asarray(lam), np.asarray(vec).reshape(6, 6)
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(vec)), what
    assert np.all(np.diff(lam) >= 0), (what, lam)
    mu, W = np.linalg.eigh(H)
    ref_orth, ref_res = eig_residuals(H, mu, W.T)
    fro = float(np.linalg.norm(H))
    orth, res = eig_residuals(H, lam, vec)
    print(f"{what}: ||VV^T - I|| {orth:.3g} (numpy {ref_orth:.3g}), residual {res:.3g} (numpy {ref_res:.3g}), ||H||_F {fro:.3g}")
    assert orth <= 16 * max(ref_orth, 8 * EPS * min(1.0, fro)), (what, orth, ref_orth)
    assert res <= 16 * max(ref_res, 8 * EPS * fro), (what, res, ref_res, fro)
    for i in range(6):  # largest-magnitude component (lowest index on ties) positive
        k = int(np.argmax(np.abs(vec[i])))
        assert vec[i, k] > 0, (what, i, vec[i])
    return mu


def covariance_numpy(H, weighted_sq_error, n_rows, rcond=1e-12):
    """sigma^2 pinv(H) with numpy's own pseudo-inverse (eigenvalues at or below rcond * largest are dropped)"""
    return weighted_sq_error / (n_rows - 6) * np.linalg.pinv(np.asarray(H).reshape(6, 6), rcond=rcond, hermitian=True)


# ---- the corridor: walls x = +-2, floor and ceiling z = +-1.5, no end walls; nothing constrains the motion along y -------
def _slice(y, shift):
    """one cross-section: 8 points per wall and per floor / ceiling strip (32 planar), 4 junction-line points (edge)"""
    zs, xs = np.linspace(-1.05, 1.05, 8), np.linspace(-1.4, 1.4, 8)
    planar = [[sx * 2.0, y, z] for sx in (-1, 1) for z in zs] + [[x, y, sz * 1.5] for sz in (-1, 1) for x in xs]
    edge = [[sx * 2.0, y, sz * 1.5] for sx in (-1, 1) for sz in (-1, 1)]
    return np.array(edge) + shift, np.array(planar) + shift


def _end_wall(n_x, n_z, y, shift):
    xs, zs = np.linspace(-1.5, 1.5, n_x), np.linspace(-1.0, 1.0, n_z)
    return np.array([[x, y, z] for x in xs for z in zs]) + shift


def corridor(end_wall=False):
    """(src_edge, src_planar, tgt_edge, tgt_planar): target 121 slices y in [-15, 15], source 49 slices y in [-12, 12] shifted
    by (-0.01, -0.07, 0.01); with end_wall a 20 x 20 wall at y = 15 in the target (400 points) and the 10 x 20 patch of it the
    source sees (200 points, shifted like the rest of the source)."""
    shift = np.array([-0.01, -0.07, 0.01])
    tgt = [_slice(y, 0.0) for y in np.linspace(-15.0, 15.0, 121)]
    src = [_slice(y, shift) for y in np.linspace(-12.0, 12.0, 49)]
    te, tp = np.concatenate([s[0] for s in tgt]), np.concatenate([s[1] for s in tgt])
    se, sp = np.concatenate([s[0] for s in src]), np.concatenate([s[1] for s in src])
    if end_wall:
        tp = np.concatenate([tp, _end_wall(20, 20, 15.0, 0.0)])
        sp = np.concatenate([sp, _end_wall(10, 20, 15.0, shift)])
    return se, sp, te, tp
