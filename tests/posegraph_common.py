"""The rule of the pose-graph optimiser (include/loamx.h, "pose graph") in plain numpy: the pose algebra, the error of an edge,
chi2, the Huber cost and the retraction, float64 operations one at a time in the header's order (numpy's elementwise loops
round every operation on its own), so e and chi2 can be compared by bytes. No code shared with the kernels. Then the part
between the Jacobians and the final poses: the dense normal equations with their damping in longdouble, the step read back
from two sets of poses, a dense solve, textbook block-Jacobi PCG and the LM loop, with the checks of one step and of a trace
that the host-build tests and the device tests share. Also: the test graphs, the binding of tests/hostcheck_posegraph and an
independent solve by scipy."""
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


# ---- the model of a step: dense normal equations, PCG and the LM loop (loamx.h: "Normal equations" to "Inner solve") -------------
LD = np.longdouble
MIN_DIAGONAL, MIN_LAMBDA, MAX_LAMBDA = 1e-6, 1e-12, 1e12


def free_poses(n, fixed=None):
    """indices of the poses that are variables (fixed None: pose 0 alone is fixed)"""
    fx = np.zeros(n, dtype=bool)
    if fixed is None:
        fx[:1] = True
    else:
        fx[:] = np.asarray(fixed) != 0
    return np.flatnonzero(~fx)


def dense_system(poses, edges, fixed, lam, huber_delta, lin, removed=()):
    """-> (H, g, free): H = sum w J^T Omega J + damping and g = sum w J^T Omega e over the edges, in longdouble, with the rows
    and columns of the fixed poses (and of `removed`, poses that left the system) dropped; free: the poses that remain, in
    order. A, B, e and w are the linearisation records `lin`; huber_delta only says which weight they must carry."""
    n = len(poses)
    assert len(lin) == len(edges)
    assert huber_delta > 0.0 or (lin["weight"] == 1.0).all()
    H, g = np.zeros((6 * n, 6 * n), dtype=LD), np.zeros(6 * n, dtype=LD)
    om = mirrored(edges["information"]).astype(LD)
    for k in range(len(edges)):
        a, b = 6 * int(edges["a"][k]), 6 * int(edges["b"][k])
        J = np.zeros((6, 6 * n), dtype=LD)
        J[:, a:a + 6], J[:, b:b + 6] = lin["A"][k], lin["B"][k]
        cols = np.r_[a:a + 6, b:b + 6]
        wOJ = LD(lin["weight"][k]) * (om[k] @ J[:, cols])
        H[np.ix_(cols, cols)] += J[:, cols].T @ wOJ
        g[cols] += wOJ.T @ lin["e"][k].astype(LD)
    d = np.diagonal(H).copy()
    H[np.arange(6 * n), np.arange(6 * n)] = d + LD(lam) * np.maximum(d, LD(MIN_DIAGONAL))
    free = np.setdiff1d(free_poses(n, fixed), np.asarray(removed, dtype=np.int64))
    idx = (6 * free[:, None] + np.arange(6)).ravel()
    return H[np.ix_(idx, idx)], g[idx], free


def step_of(poses_before, poses_after):
    """the increment (n, 6) that the retraction turned into poses_after: D = inv(T) o T', omega = 2 D_xyz / D_w, tau = t_D
    (longdouble: the poses are float64, the read-back adds no rounding of that size)"""
    T = tuple(np.asarray(poses_before, dtype=np.float64)[..., k].astype(LD) for k in range(7))
    U = tuple(np.asarray(poses_after, dtype=np.float64)[..., k].astype(LD) for k in range(7))
    qi = (-T[0], -T[1], -T[2], T[3])
    D = quat_mul(qi, U[:4])
    tau = quat_rotate(qi, tuple(U[4 + k] - T[4 + k] for k in range(3)))
    return np.stack([LD(2) * D[0] / D[3], LD(2) * D[1] / D[3], LD(2) * D[2] / D[3], tau[0], tau[1], tau[2]], axis=-1)


def dense_step(H, g):
    """x of H x = -g: a float64 solve and one refinement step with the residual formed in longdouble"""
    H64 = H.astype(np.float64)
    x = np.linalg.solve(H64, -g.astype(np.float64)).astype(LD)
    r = -g - H @ x
    return x + np.linalg.solve(H64, r.astype(np.float64)).astype(LD)


def block_inverses(H, dtype=LD):
    """the inverses of the 6 x 6 diagonal blocks of H in `dtype` (float64 inverse, two Newton steps X <- X + X (I - M X))"""
    out = []
    for i in range(0, len(H), 6):
        M = H[i:i + 6, i:i + 6].astype(dtype)
        X = np.linalg.inv(M.astype(np.float64)).astype(dtype)
        for _ in range(2):
            X = X + X @ (np.eye(6, dtype=dtype) - M @ X)
        out.append(X)
    return out


def precondition(Minv, r):
    return np.concatenate([Minv[i] @ r[6 * i:6 * i + 6] for i in range(len(Minv))])


def pcg_model(H, g, k, tol, dtype=LD):
    """Textbook block-Jacobi PCG on H x = -g from x = 0 -> (x, iterations, why): stops at r.z <= tol^2 r0.z0 ("tolerance"),
    after k iterations ("cap"), or at p.q <= 0, where it keeps x ("curvature")."""
    H, g = H.astype(dtype), g.astype(dtype)
    Minv = block_inverses(H, dtype)
    x, r = np.zeros_like(g), -g
    z = precondition(Minv, r)
    p, rz_old, rz0, it = None, None, None, 0
    while True:
        rz = r @ z
        if it == 0:
            rz0 = rz
        if not rz > dtype(tol) * dtype(tol) * rz0:
            return x, it, "tolerance"
        p = z if it == 0 else z + (rz / rz_old) * p
        q = H @ p
        pq = p @ q
        if not pq > 0:
            return x, it, "curvature"
        alpha = rz / pq
        x, r = x + alpha * p, r - alpha * q
        z = precondition(Minv, r)
        rz_old, it = rz, it + 1
        if it >= k:
            return x, it, "cap"


def residual_ratio(H, g, x):
    """sqrt(r^T M^-1 r / g^T M^-1 g) with r = -g - H x and M the diagonal blocks of H: the stopping rule on the true residual"""
    Minv = block_inverses(H)
    r = -g - H @ x
    return float(np.sqrt((r @ precondition(Minv, r)) / (g @ precondition(Minv, g))))


def preconditioned_condition(H):
    """the condition number of M^-1/2 H M^-1/2"""
    H64 = H.astype(np.float64)
    S = np.zeros_like(H64)
    for i in range(0, len(H64), 6):
        w, v = np.linalg.eigh(H64[i:i + 6, i:i + 6])
        S[i:i + 6, i:i + 6] = (v / np.sqrt(w)) @ v.T
    ev = np.linalg.eigvalsh(S @ H64 @ S)
    return float(ev[-1] / ev[0])


def energy_distance(H, x, x_ref):
    """||x - x_ref||_H / ||x_ref||_H"""
    d = x - x_ref
    return float(np.sqrt((d @ (H @ d)) / (x_ref @ (H @ x_ref))))


def apply_step(poses, free, x):
    d = np.zeros((len(poses), 6))
    d[free] = np.asarray(x, dtype=np.float64).reshape(-1, 6)
    return retract(poses, d)


def lm_model(poses, edges, fixed=None, linearize=None, **params):
    """The outer loop of loamx.h with dense_step as the inner solve and graph_cost for the costs -> one record per iteration:
    accepted, lambda (after the decision), cost (after it), c0, c1, max_update, termination (None while the solve goes on).
    linearize(poses, edges, huber_delta) gives the records (default: the host build's)."""
    P = dict(DEFAULTS)
    P.update(params)
    linearize = linearize or host_linearize
    poses = np.array(poses, dtype=np.float64)
    lam, hd = P["initial_lambda"], P["huber_delta"]
    c0 = graph_cost(poses, edges, hd)
    trace = []
    for it in range(P["max_iterations"]):
        H, g, free = dense_system(poses, edges, fixed, lam, hd, linearize(poses, edges, hd))
        x = dense_step(H, g)
        cand = apply_step(poses, free, x)
        c1, m = graph_cost(cand, edges, hd), float(np.abs(x).max())
        rec = dict(accepted=False, c0=c0, c1=c1, max_update=m, termination=None)
        if m <= P["step_tolerance"]:
            rec["termination"] = STEP_CONVERGED
        elif c1 < c0:
            rec["accepted"] = True
            lam = max(lam / 10.0, MIN_LAMBDA)
            if c0 - c1 <= P["cost_tolerance"] * c0:
                rec["termination"] = COST_CONVERGED
            poses, c0 = cand, c1
        else:
            lam = 10.0 * lam
            if lam > MAX_LAMBDA:
                rec["termination"] = LAMBDA_OVERFLOW
        if rec["termination"] is None and it + 1 >= P["max_iterations"]:
            rec["termination"] = MAX_ITERATIONS
        rec["lambda"], rec["cost"] = lam, c0
        trace.append(rec)
        if rec["termination"] is not None:
            break
    return trace


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


def hub_graph(degree, seed):
    """pose 0 sees every other pose; the others form a chain"""
    poses, edges, truth = chain_graph(degree + 1, 0, seed)
    rng = np.random.default_rng(seed + 1)
    pairs = [(0, i) if i % 3 else (i, 0) for i in range(2, degree + 1)]
    star = make_edges(pairs, measured(truth, pairs, rng, 0.001, 0.01), np.diag([900.0] * 3 + [200.0] * 3))
    return poses, np.concatenate([edges, star]), truth


def _ring40_fixed():
    fx = np.zeros(40, np.uint8)
    fx[[7, 22]] = 1
    return fx


def _ring40_information():
    poses, edges, _ = chain_graph(40, 3, seed=20, closed=True)
    rng = np.random.default_rng(21)
    edges = edges.copy()
    edges["information"] = np.stack([rand_information(rng) for _ in edges])
    return poses, edges, None, 0.0


def _ring40_outlier():
    poses, edges, _ = chain_graph(40, 3, seed=20, closed=True)
    edges = edges.copy()
    edges["a_T_b"][-1, 4] += 5.0
    return poses, edges, None, 1.0


def _backwards_and_duplicated():
    poses, edges, truth = chain_graph(20, 4, 8, closed=True)
    back = make_edges([(8, 7)], measured(truth, [(8, 7)], np.random.default_rng(9)), np.diag([100.0] * 6))  # the reverse of edge 7
    return poses, np.concatenate([edges, edges[[3, 3, 21]], back]), None, 0.0


# the graphs of the step tests -> (poses, edges, fixed, huber_delta)
STEP_GRAPHS = {
    "ring12": lambda: chain_graph(12, 2, seed=30, closed=True)[:2] + (None, 0.0),
    "ring40": lambda: chain_graph(40, 3, seed=20, closed=True)[:2] + (None, 0.0),
    "ring40_fixed_7_22": lambda: chain_graph(40, 3, seed=20, closed=True)[:2] + (_ring40_fixed(), 0.0),
    "full8": lambda: full_graph(8, seed=11)[:2] + (None, 0.0),
    "hub30": lambda: hub_graph(30, 6)[:2] + (None, 0.0),
    "ring40_information": _ring40_information,
    "ring40_outlier_huber": _ring40_outlier,
    "backwards_duplicated": _backwards_and_duplicated,
    "hub300": lambda: hub_graph(300, 6)[:2] + (None, 0.0),
}


def shaken_ring12(seed=35):
    """ring12 pushed off by 0.75 rad / 1.5 m per pose: far enough that the first two LM steps are rejected (at 0.5 rad / 1 m
    the model accepts every step, whatever the seed and the initial lambda)"""
    poses, edges, _ = chain_graph(12, 2, seed=30, closed=True)
    rng = np.random.default_rng(seed)
    poses = poses.copy()
    poses[1:] = retract(poses[1:], np.concatenate([0.75 * rng.normal(size=(11, 3)), 1.5 * rng.normal(size=(11, 3))], axis=1))
    return poses, edges


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


# ---- the checks of one LM step, shared by the host-build tests and the device tests ---------------------------------------------
# Preconditioned residual ratio of the returned step over pcg_tolerance, where PCG ended by tolerance. The recurrence's r.z is
# below tolerance^2 r0.z0 by construction; the true residual drifts from it by rounding. Measured on the host build, ratio /
# tolerance at 1e-8: ring12 0.999, ring40 0.573, ring40_fixed_7_22 0.828, full8 0.732, hub30 0.803, ring40_outlier_huber 0.381,
# backwards_duplicated 0.983, hub300 0.939; at 1e-12 between 0.021 (ring12) and 0.91 (ring40_fixed_7_22). ring40_information
# stops at its cap of 240 iterations with a ratio of 7.2e-5. The bound leaves a factor 2 over the tolerance itself.
RATIO_MARGIN = 2.0
# energy-norm distance to the dense step: ||x - x*||_H <= sqrt(kappa) ratio ||x*||_H (r^T H^-1 r <= r^T M^-1 r / lambda_min and
# g^T H^-1 g >= g^T M^-1 g / lambda_max of the preconditioned matrix), with a factor 10
ENERGY_MARGIN = 10.0


def check_step(name, poses, edges, fixed, huber_delta, lin, out, summary, pcg_tolerance, cap, removed=()):
    """One LM step from `poses` (lambda = DEFAULTS' initial_lambda) gave `out` and `summary`: holds it to the dense system built
    from the records `lin` (without the poses `removed`, which must not move). -> a dict of the figures, "by_tolerance" among them."""
    H, g, free = dense_system(poses, edges, fixed, DEFAULTS["initial_lambda"], huber_delta, lin, removed)
    x_ref = dense_step(H, g)
    c0 = graph_cost(poses, edges, huber_delta)
    assert graph_cost(apply_step(poses, free, x_ref), edges, huber_delta) < c0, f"{name}: the dense step does not lower the model's cost"
    assert summary["iterations"] == 1 and summary["accepted"] == 1, f"{name}: the step was rejected: {summary}"
    assert summary["termination"] == MAX_ITERATIONS
    x_all = step_of(poses, out)
    frozen = np.setdiff1d(np.arange(len(poses)), free)
    assert not np.asarray(x_all[frozen], dtype=np.float64).any(), f"{name}: a pose outside the system moved"
    x = x_all[free].ravel()
    assert abs(float(np.abs(x).max()) - summary["max_update"]) <= 1e-9 * summary["max_update"], f"{name}: max_update is not the step's"
    fig = dict(name=name, pcg_tolerance=pcg_tolerance, pcg_iterations=int(summary["pcg_iterations"]), ratio=residual_ratio(H, g, x),
               energy=energy_distance(H, x, x_ref), kappa=preconditioned_condition(H), by_tolerance=bool(summary["pcg_iterations"] < cap))
    print(f"{name} tol {pcg_tolerance:g}: {fig['pcg_iterations']} PCG iterations (cap {cap}), residual ratio {fig['ratio']:.3g} "
          f"({fig['ratio'] / pcg_tolerance:.3g} of the tolerance), energy distance {fig['energy']:.3g}, kappa {fig['kappa']:.4g}")
    if fig["by_tolerance"]:
        assert fig["ratio"] <= RATIO_MARGIN * pcg_tolerance, fig
        assert fig["energy"] <= ENERGY_MARGIN * pcg_tolerance * np.sqrt(fig["kappa"]), fig
    else:  # a truncated solve promises a descent step only
        assert float(g @ x) < 0.0, fig
        assert summary["final_cost"] < summary["initial_cost"] and graph_cost(out, edges, huber_delta) < c0, fig
    assert abs(summary["final_cost"] - graph_cost(out, edges, huber_delta)) <= 1e-12 * c0
    return fig


# Truncated steps against pcg_model: 100 times the largest relative difference between pcg_model in float64 and in longdouble
# over the cases of test_posegraph_hostcheck.py::test_the_truncated_step_is_the_models (ring12 and full8, 1, 2, 3 and 7
# iterations), measured 1.81e-15 (full8, 7 iterations). The host build's own largest distance is 2.1e-14.
TRUNCATED_REL_BOUND = 1.81e-13


def relative(x, ref):
    return float(np.abs(x - ref).max() / np.abs(ref).max())


# ---- a solve as a sequence of iterations ---------------------------------------------------------------------------------------
def _same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _bytes_of(s):
    return np.ascontiguousarray(s).tobytes()


def prefix_trace(solve, poses, edges, K, **kw):
    """Solves with max_iterations = 1..K. The prefix property by bytes: a solve of k iterations, continued for one iteration from
    its poses and its lambda, is the solve of k + 1 iterations (poses, cost, lambda, the counts summed), and a solve that has
    terminated early is not changed by a larger limit. -> per iteration (accepted, PCG iterations, lambda, cost), termination."""
    runs = [solve(poses, edges, None, max_iterations=k, **kw) for k in range(1, K + 1)]
    rows, prev = [], None
    for k, (out, s) in enumerate(runs, start=1):
        if prev is not None and prev[1]["termination"] != MAX_ITERATIONS:
            assert _same_bytes(out, prev[0]) and _bytes_of(s) == _bytes_of(prev[1]), k
            continue
        assert s["iterations"] == k
        if prev is not None:
            more, sm = solve(prev[0], edges, None, max_iterations=1, **dict(kw, initial_lambda=float(prev[1]["lambda"])))
            assert _same_bytes(more, out), k
            assert _bytes_of(sm["initial_cost"]) == _bytes_of(prev[1]["final_cost"]) and _bytes_of(s["initial_cost"]) == _bytes_of(runs[0][1]["initial_cost"])
            for f in ("final_cost", "lambda", "max_update", "termination"):
                assert _bytes_of(sm[f]) == _bytes_of(s[f]), (k, f)
            for f in ("accepted", "pcg_iterations"):
                assert prev[1][f] + sm[f] == s[f], (k, f)
        before = prev[1] if prev is not None else dict(accepted=0, pcg_iterations=0)
        rows.append((int(s["accepted"] - before["accepted"]), int(s["pcg_iterations"] - before["pcg_iterations"]), float(s["lambda"]), float(s["final_cost"])))
        prev = (out, s)
    return rows, int(prev[1]["termination"])


TRACE_KW = dict(cost_tolerance=0.1, step_tolerance=0.0)
TRACE_GRAPHS = {
    "ring12": lambda: STEP_GRAPHS["ring12"]()[:2],
    "ring40": lambda: STEP_GRAPHS["ring40"]()[:2],
    "ring12_shaken": shaken_ring12,
}


def check_trace(name, solve, linearize=None, K=8):
    """the accept / reject sequence, the lambda sequence and the termination of `solve` against lm_model; costs to 100
    pcg_tolerance relatively. No decision of the model may be marginal: the solver's costs are within 1e-6 of the model's, so
    the margin of the accept test (|c0 - c1|) and of the convergence test (|c0 - c1 - cost_tolerance c0|) must exceed 1e-4 c0."""
    poses, edges = TRACE_GRAPHS[name]()
    model = lm_model(poses, edges, None, linearize=linearize, max_iterations=K, **TRACE_KW)
    for r in model:
        assert abs(r["c0"] - r["c1"]) > 1e-4 * r["c0"] and abs(r["c0"] - r["c1"] - TRACE_KW["cost_tolerance"] * r["c0"]) > 1e-4 * r["c0"], r
    rows, termination = prefix_trace(solve, poses, edges, K, **TRACE_KW)
    print(name, "model:", "".join("A" if r["accepted"] else "r" for r in model), "solver:", rows, termination)
    assert [r[0] for r in rows] == [int(r["accepted"]) for r in model]
    assert [r[2] for r in rows] == [r["lambda"] for r in model]
    assert termination == model[-1]["termination"]
    for row, r in zip(rows, model):
        assert abs(row[3] - r["cost"]) <= 100.0 * DEFAULTS["pcg_tolerance"] * r["cost"], (row, r)
    return [int(r["accepted"]) for r in model]
