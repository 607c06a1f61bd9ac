"""Scenes and thresholds of the registration parameter-range tests (test_reg_params_hostcheck.py on the CPU oracle,
test_gpu_reg_params.py on the GPU). Feature sets, not scans, in the style of _scene in test_gpu_shapes.py: the target is a few
noisy planes and lines, the source a moved noisy subset. numpy only, seeded. Everything derived from the oracle (quantile
thresholds of the plane gate, the convergence sequence, the association counts) is computed here once, from the oracle module
handed in, so that the CPU test asserts the margins of exactly the numbers the GPU test uses."""
import functools

import numpy as np

IDENT = np.array([0, 0, 0, 1.0, 0, 0, 0])
INF, NAN, DBL_MAX = float("inf"), float("nan"), float(np.finfo(np.float64).max)
REG_FIELDS = ("num_edge_neighbors", "max_edge_neighbor_dist", "min_line_fit_points", "min_line_condition_number",
              "num_plane_neighbors", "max_plane_neighbor_dist", "min_plane_fit_points", "max_avg_point_plane_dist",
              "max_iterations", "rotation_convergence_thresh", "position_convergence_thresh", "min_associations")
DEFAULTS = dict(zip(REG_FIELDS, (5, 1.0, 3, 10.0, 5, 2.0, 4, 0.1, 10, 1e-3, 1e-2, 100)))


def pose7(angle, axis, t):
    """[qx qy qz qw tx ty tz] of a rotation by `angle` about `axis` and the translation t"""
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    return np.array([*(np.sin(angle / 2) * axis), np.cos(angle / 2), *np.asarray(t, dtype=np.float64)])


def rotation(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def act(pose, pts):
    return np.asarray(pts, dtype=np.float64).reshape(-1, 3) @ rotation(pose[:4]).T + pose[4:]


def _planes(rng, n, half, noise):
    """n points on three planes of a room corner (near-orthogonal normals: all six degrees of freedom are held)"""
    parts = []
    for axis in range(3):
        nrm = np.eye(3)[axis] + rng.normal(size=3) * 0.15
        nrm /= np.linalg.norm(nrm)
        u = np.cross(nrm, np.eye(3)[(axis + 1) % 3])
        u /= np.linalg.norm(u)
        v = np.cross(nrm, u)
        m = n // 3 + (axis < n % 3)
        o = nrm * rng.uniform(2.0, 3.0) * (-1) ** axis
        parts.append(o + np.outer(rng.uniform(-half, half, m), u) + np.outer(rng.uniform(-half, half, m), v) + rng.normal(size=(m, 3)) * noise)
    return np.concatenate(parts)


def _lines(rng, n, half, noise):
    parts = []
    for axis in range(3):
        d = np.eye(3)[axis] + rng.normal(size=3) * 0.2
        d /= np.linalg.norm(d)
        m = n // 3 + (axis < n % 3)
        parts.append(rng.normal(size=3) * 2.0 + np.outer(np.sort(rng.uniform(-half, half, m)), d) + rng.normal(size=(m, 3)) * noise)
    return np.concatenate(parts)


def _sets(*arrs):
    out = tuple(np.ascontiguousarray(a, dtype=np.float64) for a in arrs)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def room(seed=2, n_e=260, n_p=2700, angle=0.2, shift=0.8, half=2.5, keep=0.9, tgt_noise=0.02, src_noise=0.003):
    """(src_edge, src_planar, tgt_edge, tgt_planar): the source is the kept share of the target, moved by a rotation of
    `angle` rad and a translation of `shift` m and jittered. Read-only arrays, computed once per argument set."""
    rng = np.random.default_rng(seed)
    te, tp = _lines(rng, n_e, half, tgt_noise * 0.3), _planes(rng, n_p, half, tgt_noise)
    T = pose7(angle, rng.normal(size=3), rng.normal(size=3))
    T[4:] *= shift / max(np.linalg.norm(T[4:]), 1e-300)
    se, sp = te[rng.random(len(te)) < keep], tp[rng.random(len(tp)) < keep]
    se = act(T, se) + rng.normal(size=se.shape) * src_noise * 0.3
    sp = act(T, sp) + rng.normal(size=sp.shape) * src_noise
    return _sets(se, sp, te, tp)


def binding_room():
    """the scene of the binding parameter sets: a motion small enough for their tight radii"""
    return room(seed=2, angle=0.08, shift=0.4, tgt_noise=0.03)


def small_room():
    """about 60 + 300 points: the scene of the 1000-iteration run"""
    return room(seed=5, n_e=66, n_p=330, angle=0.01, shift=0.05, half=1.0)


def same_room():
    """a scene registered against itself"""
    se, sp, te, tp = room()
    return _sets(te, tp, te, tp)


DECOY_RADIUS = 0.3


@functools.lru_cache(maxsize=None)
def decoy(seed=2, n_p=2400, half=1.5, n_patch_tgt=1200, n_patch_src=260, shift=0.25):
    """The mid-run exit of min_associations. Target = room (dense enough for the tight plane radius DECOY_RADIUS) plus a dense
    decoy patch in the plane z = 0 at the room's centre (no lever arm); source = the room moved by t = (0, 0, shift) (plus a
    small rotation), plus patch points lifted off the patch by d in (0.02, 0.28) against t: |d| < radius < |d + t|. The patch
    associates at the identity and falls out of reach, point by point, as the room pulls the estimate over."""
    rng = np.random.default_rng(seed)
    te, tp = _lines(rng, 180, half, 0.003), _planes(rng, n_p, half, 0.004)
    T = pose7(0.02, rng.normal(size=3), [0.0, 0.0, shift])
    se, sp = act(T, te[rng.random(len(te)) < 0.9]), act(T, tp[rng.random(len(tp)) < 0.9])
    se, sp = se + rng.normal(size=se.shape) * 0.001, sp + rng.normal(size=sp.shape) * 0.002
    patch = np.column_stack([rng.uniform(-0.35, 0.35, n_patch_tgt), rng.uniform(-0.35, 0.35, n_patch_tgt), np.zeros(n_patch_tgt)])
    lifted = np.column_stack([rng.uniform(-0.25, 0.25, n_patch_src), rng.uniform(-0.25, 0.25, n_patch_src),
                              -rng.uniform(0.02, 0.28, n_patch_src)])
    return _sets(se, np.concatenate([sp, lifted]), te, np.concatenate([tp, patch]))


# ---- parameters ------------------------------------------------------------------------------------------------------------
def params(cls, **over):
    """a parameter struct of class `cls` (oracle_lib.RegParams, capi.RegistrationParams, hostcheck_lib.RegParams) with the
    defaults of the reference and the fields of `over`"""
    v = dict(DEFAULTS)
    unknown = set(over) - set(v)
    assert not unknown, unknown
    v.update(over)
    return cls(*[v[f] for f in REG_FIELDS])


# ---- derived from the oracle -----------------------------------------------------------------------------------------------
_cache = {}


def cached(fn):
    """per (function, arguments) cache that does not key on the oracle module"""
    @functools.wraps(fn)
    def wrapped(oracle, *a):
        key = (fn.__name__,) + a
        if key not in _cache:
            _cache[key] = fn(oracle, *a)
        return _cache[key]
    return wrapped


def neighbour_lists(oracle, src, tgt, pose, k, radius):
    tree = oracle.KDTree(tgt)
    return [tree.knn(m, k, radius).astype(np.int64) for m in act(pose, src)]


def avgs_of(oracle, sp, tp, k, radius, min_pts):
    """(avg (n,) of every source plane at the identity from oracle.fit_plane on the oracle's neighbour list, NaN where the list
    is shorter than min_pts; the lists)"""
    lists = neighbour_lists(oracle, sp, tp, IDENT, k, radius)
    return np.array([oracle.fit_plane(tp[l])[2] if len(l) >= min_pts else np.nan for l in lists]), lists


@cached
def plane_avgs(oracle):
    """avgs_of room() under the default parameters"""
    se, sp, te, tp = room()
    return avgs_of(oracle, sp, tp, DEFAULTS["num_plane_neighbors"], DEFAULTS["max_plane_neighbor_dist"], DEFAULTS["min_plane_fit_points"])


MIN_GAP = 1e-9  # 1000 x the plain 1e-12 fit bar of test_gpu_direct.py


def gap_threshold(avg, q):
    """(threshold, value below, value above) near the q quantile of the avg values: the midpoint of the first gap of at least
    MIN_GAP between adjacent sorted values at or above the quantile"""
    s = np.sort(avg[~np.isnan(avg)])
    i = int(q * len(s))
    while s[i + 1] - s[i] < MIN_GAP:
        i += 1
    return float(0.5 * (s[i] + s[i + 1])), float(s[i]), float(s[i + 1])


@cached
def gap_thresholds(oracle):
    """the gap thresholds of room() near the 10 %, 50 % and 90 % quantile"""
    return [gap_threshold(plane_avgs(oracle)[0], q) for q in (0.1, 0.5, 0.9)]


@cached
def edge_plane(oracle):
    """index of the source plane whose avg is the on-the-edge threshold: the first plane from the median up that no other plane
    shares its oracle avg with (the GPU test takes the threshold itself from the hostcheck value of that plane)"""
    avg, _ = plane_avgs(oracle)
    order = np.argsort(np.where(np.isnan(avg), np.inf, avg))
    n = int((~np.isnan(avg)).sum())
    for i in order[n // 2:n]:
        if (avg == avg[i]).sum() == 1:
            return int(i)
    raise AssertionError("no plane with an avg of its own")


def changes(oracle, updates):
    """(angle change, position change) of every update (pose7): what registration-inl.h:68-69 compares"""
    return ([oracle.quat_angular_distance(np.asarray(u)[:4], [0, 0, 0, 1.0]) for u in updates],
            [float(np.linalg.norm(np.asarray(u)[4:])) for u in updates])


def oracle_updates(info):
    return [np.array(list(a.update)) for a in info]


def sequence_of(oracle, sets, **over):
    """(a, p): the oracle's per-iteration angle and position changes with both thresholds 0 and max_iterations 8"""
    prm = params(oracle.RegParams, **{**over, "rotation_convergence_thresh": 0.0, "position_convergence_thresh": 0.0, "max_iterations": 8})
    _, term, iters, info = oracle.register_features(*sets, None, prm, want_info=True)
    assert (term, iters) == (oracle.MAX_ITER, 8)
    return changes(oracle, oracle_updates(info))


@cached
def convergence_sequence(oracle):
    return sequence_of(oracle, room())


def between(seq, j):
    """the geometric mean of seq[j - 1] and seq[j]: first satisfied (seq[i] < threshold) at iteration j"""
    return float(np.sqrt(seq[j] * seq[j - 1]))


@cached
def convergence_cases(oracle):
    """{name: (rotation threshold, position threshold)} of section D, cases 1 - 3, from the sequences of room()"""
    a, p = convergence_sequence(oracle)
    return {
        "rot_binds_1": (between(a, 1), INF), "rot_binds_2": (between(a, 2), INF),
        "pos_binds_1": (INF, between(p, 1)), "pos_binds_2": (INF, between(p, 2)),
        # rot satisfied from iteration 1 and pos only from iteration 3, then the roles exchanged
        "rot_1_pos_3": (between(a, 1), between(p, 3)), "rot_3_pos_1": (between(a, 3), between(p, 1)),
        # (on this scene both of those stop after four iterations, and so do they with their two numbers exchanged: p is about
        # four times a. The next two stop elsewhere once their numbers are exchanged - SWAP_SHOWN_BY)
        "rot_2_pos_1": (between(a, 2), between(p, 1)), "rot_1_pos_1": (between(a, 1), between(p, 1)),
    }


SWAP_SHOWN_BY = ("rot_2_pos_1", "rot_1_pos_1")
INIT_POSE = pose7(0.05, [1.0, -2.0, 0.5], [0.1, -0.05, 0.08])  # a non-identity initial pose
INIT_POSE.setflags(write=False)
IDENT.setflags(write=False)


def iterations_by_sequence(a, p, rot, pos, max_iterations):
    """(iterations, converged) that registration-inl.h:28-76 gives for the change sequences a, p"""
    for i in range(min(len(a), max_iterations)):
        if a[i] < rot and p[i] < pos:
            return i + 1, True
    return max_iterations, False


def thresholds_used(cases):
    """[(name, which sequence, threshold)] of every finite threshold of `cases`"""
    out = []
    for name, (rot, pos) in cases.items():
        out += [(name, "a", rot)] if np.isfinite(rot) else []
        out += [(name, "p", pos)] if np.isfinite(pos) else []
    return out


def margins(seq, thr):
    """(value below, value above, smallest absolute distance, smallest ratio) of a threshold inside a decreasing sequence"""
    seq = np.asarray(seq, dtype=np.float64)
    below, above = seq[seq < thr].max(), seq[seq >= thr].min()
    return float(below), float(above), float(min(thr - below, above - thr)), float(min(thr / below if below > 0 else INF, above / thr))


DECOY_OVER = dict(max_plane_neighbor_dist=DECOY_RADIUS, rotation_convergence_thresh=0.0, position_convergence_thresh=0.0, max_iterations=4)


@cached
def decoy_counts(oracle):
    """association count (edges + planes) of every iteration of the oracle on decoy() under DECOY_OVER, min_associations 0"""
    prm = params(oracle.RegParams, **{**DECOY_OVER, "min_associations": 0})
    _, _, _, info = oracle.register_features(*decoy(), None, prm, want_info=True)
    return [int(i.n_edge_assoc) + int(i.n_plane_assoc) for i in info]


# ---- section C: neighbour counts and fit-point minima, at the pose the oracle registers room() to ----------------------------
@cached
def registered_pose(oracle):
    return np.asarray(oracle.register_features(*room())[0], dtype=np.float64)


FIT_K = {False: 4, True: 6}             # is_plane -> k
FIT_RADIUS = {False: 0.12, True: 0.22}  # is_plane -> a radius that leaves some queries short of k neighbours


def short_and_full(oracle, is_plane):
    """(queries of room() at the registered pose with fewer than k neighbours inside the radius, queries with all k)"""
    se, sp, te, tp = room()
    src, tgt = (sp, tp) if is_plane else (se, te)
    n = np.array([len(l) for l in neighbour_lists(oracle, src, tgt, registered_pose(oracle), FIT_K[is_plane], FIT_RADIUS[is_plane])])
    return int((n < FIT_K[is_plane]).sum()), int((n == FIT_K[is_plane]).sum())


# ---- section F: one batch, every ending --------------------------------------------------------------------------------------
def dense_room(seed, angle, shift, n_e=180, n_p=2400):
    """a room dense enough for the tight plane radius of the decoy scene"""
    return room(seed=seed, n_e=n_e, n_p=n_p, angle=angle, shift=shift, half=1.5, tgt_noise=0.004, src_noise=0.002)


BATCH_OVER = dict(num_edge_neighbors=4, min_plane_fit_points=5, max_plane_neighbor_dist=DECOY_RADIUS, max_iterations=4,
                  rotation_convergence_thresh=2e-4, position_convergence_thresh=2e-3, min_associations=1100)
CONVERGED, MAX_ITER, INSUFFICIENT = 0, 1, 2
BATCH_ENDINGS = [(CONVERGED, 1), (CONVERGED, 2), (CONVERGED, 3), (MAX_ITER, 4), (INSUFFICIENT, 0), (INSUFFICIENT, 1)]
# (scene, (termination, iterations) the oracle gives under BATCH_OVER: asserted by test_reg_params_hostcheck.py)
BATCH = [
    (lambda: dense_room(11, 0.0, 0.0), (CONVERGED, 1)),
    (lambda: dense_room(11, 0.15, 0.5), (MAX_ITER, 4)),
    (lambda: dense_room(11, 0.01, 0.03), (CONVERGED, 2)),
    (lambda: decoy(n_p=900, half=1.0), (INSUFFICIENT, 1)),       # the patch is out of reach after the first update
    (lambda: dense_room(11, 0.04, 0.15), (CONVERGED, 3)),
    (lambda: dense_room(15, 0.01, 0.03, 60, 600), (INSUFFICIENT, 0)),  # fewer features than min_associations
    (lambda: dense_room(11, 0.2, 0.6), (MAX_ITER, 4)),
    (lambda: dense_room(12, 0.06, 0.25), (CONVERGED, 3)),
    (lambda: dense_room(13, 0.0, 0.0), (CONVERGED, 1)),
    (lambda: dense_room(11, 0.1, 0.4), (CONVERGED, 4)),
    (lambda: dense_room(12, 0.002, 0.01), (CONVERGED, 2)),
]


# ---- section G: all twelve fields off their defaults and pairwise distinct ---------------------------------------------------
def signature(oracle, sets, prm):
    """what a binding must carry through: (termination, iterations, (n_edge, n_plane) of the first iteration, pose)"""
    pose, term, iters, info = oracle.register_features(*sets, None, prm, want_info=True)
    first = (int(info[0].n_edge_assoc), int(info[0].n_plane_assoc)) if iters else None
    return term, iters, first, pose


def differs(oracle, s1, s2):
    """two signatures differ by something a GPU run held to the oracle cannot miss: the termination, the iteration count, the
    association counts of the first iteration (the estimate there is the initial pose, bit for bit), or a pose 100 x the 1e-5 bar apart"""
    if s1[:3] != s2[:3]:
        return True
    d = oracle.pose_compose(oracle.pose_inverse(s1[3]), s2[3])
    return oracle.quat_angular_distance(d[:4], [0, 0, 0, 1.0]) > 1e-3 or float(np.linalg.norm(d[4:])) > 1e-3


@cached
def binding_sets(oracle):
    """{name: the twelve fields} of the three parameter sets of section G on room(). In every set all twelve fields are off their
    defaults and pairwise distinct. No ONE set can make every field matter:
      - min_line_condition_number rejects nothing unless it is +inf (the condition number is always DBL_MAX), and at +inf no edge
        associates, so the three edge fields are dead;
      - max_iterations is read only by a run that has not converged, and with decreasing change sequences a run that has not
        converged cannot be made to converge by loosening the rotation threshold alone AND by loosening the position threshold
        alone (the first needs p_i < pos at an iteration where a_i >= rot, the second a_j < rot where p_j >= pos: i < j and j < i);
      - min_associations above the default matters only to a run that ends INSUFFICIENT, which reads no convergence threshold.
    So: "converged" makes the nine remaining fields matter, "insufficient" (the line gate at +inf, min_associations one above the
    plane count) the line gate and min_associations, "max_iter" max_iterations."""
    sets = binding_room()
    base = dict(num_edge_neighbors=7, max_edge_neighbor_dist=0.45, min_line_fit_points=6, min_line_condition_number=DBL_MAX,
                num_plane_neighbors=9, max_plane_neighbor_dist=0.6, min_plane_fit_points=8, max_iterations=11, min_associations=37)
    avg, _ = avgs_of(oracle, sets[1], sets[3], 9, 0.6, 8)
    base["max_avg_point_plane_dist"] = gap_threshold(avg, 0.5)[0]
    a, p = sequence_of(oracle, sets, **base)
    # rot first holds at iteration 1 (the default 1e-3 later), pos at iteration 0 (the default 1e-2 later): two iterations
    base["rotation_convergence_thresh"], base["position_convergence_thresh"] = between(a, 1), 2.0 * p[0]
    n_plane = signature(oracle, sets, params(oracle.RegParams, **base))[2][1]
    return {"converged": base, "insufficient": {**base, "min_line_condition_number": INF, "min_associations": n_plane + 1},
            "max_iter": {**base, "max_iterations": 1}}


BINDING_COVERS = {"converged": ("num_edge_neighbors", "max_edge_neighbor_dist", "min_line_fit_points", "num_plane_neighbors",
                                "max_plane_neighbor_dist", "min_plane_fit_points", "max_avg_point_plane_dist",
                                "rotation_convergence_thresh", "position_convergence_thresh"),
                  "insufficient": ("min_line_condition_number", "min_associations"), "max_iter": ("max_iterations",)}
