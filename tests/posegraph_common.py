"""The rule of the pose-graph optimiser (include/loamx.h, "pose graph") in plain numpy: the pose algebra, the error of an edge,
chi2, the Huber cost and the retraction, float64 operations one at a time in the header's order (numpy's elementwise loops
round every operation on its own), so e and chi2 can be compared by bytes. No code shared with the kernels. Also: the
test graphs, the binding of tests/hostcheck_posegraph and an independent solve by scipy."""
import ctypes as C
import os
import subprocess

import numpy as np

EDGE_DTYPE = np.dtype([("a", np.uint32), ("b", np.uint32), ("a_T_b", np.float64, 7), ("information", np.float64, (6, 6))])
SUMMARY_DTYPE = np.dtype([("initial_cost", np.float64), ("final_cost", np.float64), ("lambda", np.float64), ("max_update", np.float64),
                          ("iterations", np.uint32), ("accepted", np.uint32), ("pcg_iterations", np.uint32), ("termination", np.uint32),
                          ("n_bad_edges", np.uint32), ("reserved", np.uint32)])
LIN_DTYPE = np.dtype([("e", np.float64, 6), ("chi2", np.float64), ("weight", np.float64), ("A", np.float64, (6, 6)), ("B", np.float64, (6, 6))])
COST_CONVERGED, STEP_CONVERGED, MAX_ITERATIONS, LAMBDA_OVERFLOW, NOTHING_TO_DO, BAD_INPUT = range(6)
DEFAULTS = dict(max_iterations=20, max_pcg_iterations=500, pcg_tolerance=1e-8, initial_lambda=1e-4, cost_tolerance=1e-9,
                step_tolerance=1e-10, huber_delta=0.0)


# ---- the model: arrays of poses (..., 7) --------------------------------------------------------------------------------------
def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def quat_rotate(q, v):
    """q (x, y, z, w) and v as tuples of arrays: v + w (2 u x v) + u x (2 u x v)"""
    u = (q[0], q[1], q[2])
    uv = _cross(u, v)
    uv = tuple(c + c for c in uv)
    cc = _cross(u, uv)
    return tuple((v[k] + q[3] * uv[k]) + cc[k] for k in range(3))


def quat_mul(a, b):
    x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1]
    y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2]
    z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0]
    w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]
    return (x, y, z, w)


def _cols(T):
    T = np.asarray(T, dtype=np.float64)
    return tuple(T[..., k] for k in range(7))


def _stack(cols):
    return np.stack(np.broadcast_arrays(*cols), axis=-1)


def compose(a, b):
    a, b = _cols(a), _cols(b)
    q = quat_mul(a[:4], b[:4])
    r = quat_rotate(a[:4], b[4:])
    return _stack(q + tuple(a[4 + k] + r[k] for k in range(3)))


def inverse(T):
    T = _cols(T)
    q = (-T[0], -T[1], -T[2], T[3])
    r = quat_rotate(q, T[4:])
    return _stack(q + tuple(-c for c in r))


def error(Ta, Tb, Z):
    """e (..., 6) of the edges with measurement Z between the poses Ta and Tb"""
    zhat = _cols(compose(inverse(Ta), Tb))
    Z = _cols(Z)
    qd = quat_mul(zhat[:4], (-Z[0], -Z[1], -Z[2], Z[3]))
    rt = quat_rotate(qd, Z[4:])
    s2 = 2.0 * np.where(qd[3] < 0.0, -1.0, 1.0)
    return _stack(tuple(s2 * qd[k] for k in range(3)) + tuple(zhat[4 + k] - rt[k] for k in range(3)))


def mirrored(information):
    """the matrix the rule reads: the upper triangle, mirrored"""
    m = np.asarray(information, dtype=np.float64)
    up = np.triu(m)
    return up + np.swapaxes(np.triu(m, 1), -1, -2)


def chi2(information, e):
    om = mirrored(information)
    oe = []
    for i in range(6):
        s = np.zeros(e.shape[:-1])
        for j in range(6):
            s = s + om[..., i, j] * e[..., j]
        oe.append(s)
    c = np.zeros(e.shape[:-1])
    for i in range(6):
        c = c + e[..., i] * oe[i]
    return c


def weight_cost(c2, huber_delta):
    c2 = np.asarray(c2, dtype=np.float64)
    if not huber_delta > 0.0:
        return np.ones_like(c2), c2.copy()
    chi = np.sqrt(c2)
    out = c2 > huber_delta * huber_delta
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(out, huber_delta / chi, 1.0), np.where(out, (2.0 * huber_delta) * chi - huber_delta * huber_delta, c2)


def retract(T, d):
    """T o (normalise([omega / 2, 1]), tau)"""
    d = np.asarray(d, dtype=np.float64)
    hx, hy, hz = d[..., 0] / 2.0, d[..., 1] / 2.0, d[..., 2] / 2.0
    n = np.sqrt(hx * hx + hy * hy + hz * hz + 1.0)
    return compose(T, _stack((hx / n, hy / n, hz / n, 1.0 / n, d[..., 3], d[..., 4], d[..., 5])))


def edge_errors(poses, edges):
    return error(poses[edges["a"]], poses[edges["b"]], edges["a_T_b"])


def graph_cost(poses, edges, huber_delta=0.0):
    return float(weight_cost(chi2(edges["information"], edge_errors(poses, edges)), huber_delta)[1].sum())


# ---- test graphs ------------------------------------------------------------------------------------------------------------------
def rand_quat(rng, max_angle):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = rng.uniform(-max_angle, max_angle)
    return np.concatenate([np.sin(ang / 2) * ax, [np.cos(ang / 2)]])


def rand_pose(rng, max_angle=3.0, extent=10.0):
    return np.concatenate([rand_quat(rng, max_angle), rng.uniform(-extent, extent, 3)])


def rand_information(rng, rank=6, scale=100.0):
    m = rng.normal(size=(rank, 6))
    return scale * (m.T @ m) + (np.eye(6) if rank == 6 else 0.0)


def make_edges(pairs, Z, information):
    e = np.zeros(len(pairs), dtype=EDGE_DTYPE)
    if len(pairs):
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        e["a"], e["b"] = pairs[:, 0], pairs[:, 1]
        e["a_T_b"] = Z
        e["information"] = information
    return e


def ring_truth(n, radius=10.0, rng=None):
    th = 2 * np.pi * np.arange(n) / max(n, 1)
    T = np.zeros((n, 7))
    T[:, 2], T[:, 3] = np.sin(th / 2 + np.pi / 4), np.cos(th / 2 + np.pi / 4)
    T[:, 4], T[:, 5] = radius * np.cos(th), radius * np.sin(th)
    if rng is not None:
        T[:, 6] = 0.2 * rng.normal(size=n)
    return T


def measured(truth, pairs, rng, sigma_rot=0.0, sigma_t=0.0):
    """a_T_b of the pairs from the truth by the model's own arithmetic, with noise as a right perturbation"""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    Z = compose(inverse(truth[pairs[:, 0]]), truth[pairs[:, 1]])
    if sigma_rot or sigma_t:
        d = np.concatenate([sigma_rot * rng.normal(size=(len(pairs), 3)), sigma_t * rng.normal(size=(len(pairs), 3))], axis=1)
        Z = retract(Z, d)
    return Z


def dead_reckon(truth0, Z_chain):
    """the poses a chain of odometry measurements composes from the first pose"""
    out = [np.asarray(truth0, dtype=np.float64)]
    for z in Z_chain:
        out.append(compose(out[-1], z))
    return np.stack(out)


def chain_graph(n, loops, seed, sigma_rot=0.002, sigma_t=0.02, information=None, closed=False):
    """n poses on a ring, odometry edges (i, i + 1) with noise, `loops` extra edges (listed old <- new half of the time), the
    start from dead reckoning. -> (poses, edges, truth)"""
    rng = np.random.default_rng(seed)
    truth = ring_truth(n, rng=rng)
    pairs = [(i, i + 1) for i in range(n - 1)]
    Z = measured(truth, pairs, rng, sigma_rot, sigma_t) if pairs else np.zeros((0, 7))
    poses = dead_reckon(truth[0], Z) if n else np.zeros((0, 7))
    extra = []
    if closed and n > 2:
        extra.append((n - 1, 0))
    for k in range(loops):
        a, b = sorted(rng.choice(n, size=2, replace=False))
        extra.append((int(b), int(a)) if k % 2 else (int(a), int(b)))
    if extra:
        pairs = pairs + extra
        Z = np.concatenate([Z, measured(truth, extra, rng, sigma_rot / 4, sigma_t / 4)])
    info = np.diag([2500.0, 2500.0, 2500.0, 400.0, 400.0, 400.0]) if information is None else information
    return poses, make_edges(pairs, Z, info), truth


def full_graph(n, seed, sigma_rot=0.01, sigma_t=0.05):
    rng = np.random.default_rng(seed)
    truth = np.stack([rand_pose(rng, 3.0, 5.0) for _ in range(n)])
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    Z = measured(truth, pairs, rng, sigma_rot, sigma_t)
    info = np.stack([rand_information(rng) for _ in pairs])
    poses = retract(truth, np.concatenate([0.05 * rng.normal(size=(n, 3)), 0.3 * rng.normal(size=(n, 3))], axis=1))
    poses[0] = truth[0]
    return poses, make_edges(pairs, Z, info), truth


def pose_distance(a, b):
    """(rotation angle, translation distance) between poses, up to the sign of q"""
    a, b = np.asarray(a), np.asarray(b)
    dot = np.abs((a[..., :4] * b[..., :4]).sum(-1)) / (np.linalg.norm(a[..., :4], axis=-1) * np.linalg.norm(b[..., :4], axis=-1))
    return 2 * np.arccos(np.clip(dot, 0, 1)), np.linalg.norm(a[..., 4:] - b[..., 4:], axis=-1)


# ---- the host build -------------------------------------------------------------------------------------------------------------
_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck_posegraph")
_lib = None


class Params(C.Structure):
    _fields_ = [("max_iterations", C.c_uint32), ("max_pcg_iterations", C.c_uint32), ("pcg_tolerance", C.c_double),
                ("initial_lambda", C.c_double), ("cost_tolerance", C.c_double), ("step_tolerance", C.c_double), ("huber_delta", C.c_double)]


def params(**kw):
    d = dict(DEFAULTS)
    d.update(kw)
    return Params(**d)


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", _DIR])
        _lib = C.CDLL(os.path.join(_DIR, "libhostcheck_posegraph.so"))
        _lib.hostcheck_pgo_cholesky_inverse.restype = C.c_int
    return _lib


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def host_sizes():
    out = np.zeros(4, dtype=np.uint64)
    lib().hostcheck_pgo_sizes(_vp(out))
    return tuple(int(v) for v in out)


def host_linearize(poses, edges, huber_delta=0.0):
    poses = np.ascontiguousarray(poses, dtype=np.float64)
    edges = np.ascontiguousarray(edges, dtype=EDGE_DTYPE)
    out = np.zeros(len(edges), dtype=LIN_DTYPE)
    lib().hostcheck_pgo_linearize(_vp(poses), _vp(edges), C.c_uint64(len(edges)), C.c_double(huber_delta), _vp(out))
    return out


def host_retract(T, d):
    T, d, out = np.ascontiguousarray(T, dtype=np.float64), np.ascontiguousarray(d, dtype=np.float64), np.zeros(7)
    lib().hostcheck_pgo_retract(_vp(T), _vp(d), _vp(out))
    return out


def host_optimize(poses, edges, fixed=None, **kw):
    """-> (poses, summary record) of the host build's whole solve"""
    poses = np.array(poses, dtype=np.float64).reshape(-1, 7)
    edges = np.ascontiguousarray(edges, dtype=EDGE_DTYPE)
    fx = None if fixed is None else np.ascontiguousarray(fixed, dtype=np.uint8)
    summary = np.zeros(1, dtype=SUMMARY_DTYPE)
    p = params(**kw)
    lib().hostcheck_pgo_optimize(_vp(poses), C.c_uint64(len(poses)), None if fx is None else _vp(fx), _vp(edges), C.c_uint64(len(edges)),
                                 C.byref(p), _vp(summary))
    return poses, summary[0]


# ---- an independent solve ---------------------------------------------------------------------------------------------------------
def scipy_solve(poses, edges, fixed=None):
    """scipy.optimize.least_squares on the residuals L e (L^T L = Omega), tolerances at 1e-15 -> (poses, cost)"""
    from scipy.optimize import least_squares
    from scipy.sparse import csr_matrix
    poses = np.asarray(poses, dtype=np.float64)
    n = len(poses)
    fx = np.zeros(n, dtype=bool)
    if fixed is None:
        fx[0] = True
    else:
        fx[:] = np.asarray(fixed) != 0
    free = np.flatnonzero(~fx)
    col = -np.ones(n, dtype=np.int64)
    col[free] = np.arange(len(free))
    om = mirrored(edges["information"])
    w, v = np.linalg.eigh(om)
    L = np.sqrt(np.clip(w, 0, None))[..., :, None] * np.swapaxes(v, -1, -2)  # L^T L = Omega, also when Omega is singular

    def current(xv):
        d = np.zeros((n, 6))
        d[free] = xv.reshape(-1, 6)
        return retract(poses, d)

    def res(xv):
        return np.einsum("eij,ej->ei", L, edge_errors(current(xv), edges)).ravel()

    ea, eb = edges["a"].astype(np.int64), edges["b"].astype(np.int64)
    rows = np.arange(len(edges))

    def jac(xv):
        """central differences (h = 1e-6) edge by edge: an edge depends on the twelve variables of its two poses only. (The
        solver's own differences, column by column or grouped by sparsity with its iterative trust-region solver, take minutes
        or stop far from the minimum on the 300-pose chain.)"""
        d = np.zeros((n, 6))
        d[free] = xv.reshape(-1, 6)
        Ta, Tb, h = retract(poses[ea], d[ea]), retract(poses[eb], d[eb]), 1e-6
        J = np.zeros((len(edges), 6, 6 * len(free)))
        for k in range(6):
            dk = np.zeros(6)
            dk[k] = h
            da = (error(retract(poses[ea], d[ea] + dk), Tb, edges["a_T_b"]) - error(retract(poses[ea], d[ea] - dk), Tb, edges["a_T_b"])) / (2 * h)
            db = (error(Ta, retract(poses[eb], d[eb] + dk), edges["a_T_b"]) - error(Ta, retract(poses[eb], d[eb] - dk), edges["a_T_b"])) / (2 * h)
            for ends, dv in ((ea, da), (eb, db)):
                ok = col[ends] >= 0
                J[rows[ok], :, 6 * col[ends[ok]] + k] = np.einsum("eij,ej->ei", L[ok], dv[ok])
        return csr_matrix(J.reshape(6 * len(edges), 6 * len(free)))

    # (the trust-region subproblems by LSMR run to 1e-14: at its default tolerances the solver creeps along the chain's
    # drift direction and stops far from the minimum; the dense solvers take a quarter of a minute on the 300-pose chain)
    sol = least_squares(res, np.zeros(6 * len(free)), jac=jac, method="trf", tr_solver="lsmr", tr_options=dict(atol=1e-14, btol=1e-14, maxiter=20000),
                        xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=400)
    return current(sol.x), float(2.0 * sol.cost)
