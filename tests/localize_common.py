"""Surfel localisation (include/loamx.h, "surfel localisation") for the tests: the scenes, the binding of tests/hostcheck_localize
(localize_math.h compiled by g++ with a host loop in the kernels' orders) and an independent numpy model of the rule on top of
surfel_common.SurfelMapModel. The model shares no code with the header: it evaluates all points of a cloud at once, sums with
numpy and takes the eigenpairs from numpy.linalg.eigh. Discrete outputs (the chosen candidate of every point, the counters,
used_mask, termination, iterations) are compared by equality, floats within a measured bound (tests/test_localize_hostcheck.py)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import cloudmap_common as CM
import outdoor_scenes as S
import surfel_common as M

CHUNK = 4096            # kLocChunk
CHUNK_CLOUDS = 256      # kOrgChunkClouds
CONVERGED, MAX_ITERATIONS, TOO_FEW_ROWS, NOT_FINITE = range(4)
OUT_UNUSED, OUT_NO_SURFEL, OUT_GATED, OUT_NOT_FINITE = -1, -2, -3, -4
PARAM_NAMES = ("neighborhood", "min_points", "planarity", "max_distance", "huber_delta", "max_iterations", "min_rows",
               "rotation_convergence_thresh", "position_convergence_thresh", "min_eigenvalue_per_row")
DEFAULTS = dict(neighborhood=7, min_points=5, planarity=0.1, max_distance=0.0, huber_delta=0.1, max_iterations=10, min_rows=100,
                rotation_convergence_thresh=1e-3, position_convergence_thresh=1e-2, min_eigenvalue_per_row=1e-3)
PARAMS_DTYPE = np.dtype([("neighborhood", np.uint32), ("min_points", np.uint32), ("planarity", np.float64), ("max_distance", np.float64),
                         ("huber_delta", np.float64), ("max_iterations", np.uint32), ("min_rows", np.uint32),
                         ("rotation_convergence_thresh", np.float64), ("position_convergence_thresh", np.float64),
                         ("min_eigenvalue_per_row", np.float64)])
RESULT_DTYPE = np.dtype([("pose", np.float64, 7), ("initial_cost", np.float64), ("final_cost", np.float64), ("last_rotation", np.float64),
                         ("last_translation", np.float64), ("iterations", np.uint32), ("termination", np.uint32), ("n_rows", np.uint32),
                         ("n_huber", np.uint32), ("n_no_surfel", np.uint32), ("n_gated", np.uint32), ("n_unused", np.uint32),
                         ("used_mask", np.uint32), ("n_rows_initial", np.uint32), ("reserved", np.uint32)])
INFO_DTYPE = np.dtype([("information", np.float64, (6, 6)), ("eigenvalues", np.float64, 6), ("eigenvectors", np.float64, (6, 6)),
                       ("gradient", np.float64, 6), ("weighted_sq_error", np.float64), ("n_edge", np.uint32), ("n_plane", np.uint32),
                       ("n_huber", np.uint32), ("n_dropped", np.uint32)])
HEAD_DTYPE = np.dtype([("n_vox", np.uint64), ("n_rows", np.uint64), ("stride", np.uint64), ("n_clouds", np.uint64), ("leaf", np.float64),
                       ("min_range", np.float64), ("max_range", np.float64), ("params", PARAMS_DTYPE)])
VOX_DTYPE = np.dtype([("key", np.uint64), ("s", np.uint64, 3), ("S", np.uint64, 6), ("W", np.int64, 3), ("count", np.uint32), ("first", np.uint32)])
assert PARAMS_DTYPE.itemsize == 64 and RESULT_DTYPE.itemsize == 128 and INFO_DTYPE.itemsize == 696 and HEAD_DTYPE.itemsize == 120
assert VOX_DTYPE.itemsize == 112
COUNTERS = ("n_rows", "n_huber", "n_no_surfel", "n_gated", "n_unused")
DISCRETE = COUNTERS + ("used_mask", "termination", "iterations", "n_rows_initial")
NEAR = 1e-9  # a point whose |s| or candidate distances lie this close to a decision is left out of the comparison with the model


def params(**kw):
    assert set(kw) <= set(PARAM_NAMES), kw
    return dict(DEFAULTS, **kw)


def params_record(p):
    rec = np.zeros(1, dtype=PARAMS_DTYPE)
    for n in PARAM_NAMES:
        rec[n] = p[n]
    return rec


# ---- tests/hostcheck_localize ----------------------------------------------------------------------------------------------------
HOSTCHECK_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck_localize")
_lib = None


def hostcheck_lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", HOSTCHECK_DIR])
        _lib = C.CDLL(os.path.join(HOSTCHECK_DIR, "libhostcheck_localize.so"))
        _lib.hostcheck_localize.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        _lib.hostcheck_candidate_key.argtypes = [C.c_uint64, C.c_int32, C.POINTER(C.c_uint64)]
    return _lib


def candidate_key(home, k):
    """loc_candidate_key of the header: (ok, key) of candidate k of the voxel with the packed key `home`"""
    key = C.c_uint64(0)
    ok = hostcheck_lib().hostcheck_candidate_key(int(home), int(k), C.byref(key))
    return bool(ok), key.value


def hostcheck_san_program():
    subprocess.check_call(["make", "-s", "-C", HOSTCHECK_DIR, "san"])
    return os.path.join(HOSTCHECK_DIR, "hostcheck_localize_san")


def vox_records(model):
    """the voxels of a SurfelMapModel as the host build takes them"""
    vox = np.zeros(len(model.vox), dtype=VOX_DTYPE)
    for i, (key, e) in enumerate(model.vox.items()):
        vox[i] = (key, e[1], e[2], e[3], e[4], e[5])
    return vox


def blob(model, points, offsets, poses, p):
    pts = np.ascontiguousarray(points, dtype=np.float64)  # (float32 points widen exactly, as the kernel's loads do)
    assert pts.ndim == 2 and pts.shape[1] >= 3
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(len(off) - 1, 7)
    head = np.zeros(1, dtype=HEAD_DTYPE)
    vox = vox_records(model)
    head["n_vox"], head["n_rows"], head["stride"], head["n_clouds"] = len(vox), len(pts), pts.shape[1], len(off) - 1
    head["leaf"], head["min_range"], head["max_range"], head["params"] = model.leaf, model.min_range, model.max_range, params_record(p)
    return head.tobytes() + vox.tobytes() + pts.tobytes() + off.tobytes() + poses.tobytes(), len(pts), len(off) - 1


def unpack(out, n_rows, n_clouds):
    o_res = n_clouds * 56
    o_info = o_res + n_clouds * 128
    o_chosen = o_info + n_clouds * 696
    assert len(out) == o_chosen + 4 * n_rows, (len(out), n_rows, n_clouds)
    return dict(poses=np.frombuffer(out, np.float64, n_clouds * 7, 0).reshape(n_clouds, 7).copy(),
                results=np.frombuffer(out, RESULT_DTYPE, n_clouds, o_res).copy(), info=np.frombuffer(out, INFO_DTYPE, n_clouds, o_info).copy(),
                chosen=np.frombuffer(out, np.int32, n_rows, o_chosen).copy())


def host_run(model, points, offsets, poses, p, program=None):
    """the host build on clouds `points[offsets[c]:offsets[c + 1]]` from `poses` against the voxels of a SurfelMapModel ->
    dict(poses, results, info, chosen): what the device leaves, and per point of the LAST evaluation the chosen candidate 0 .. 6 or
    OUT_*. program: the stand-alone (sanitizer) build instead of the library."""
    data, n_rows, n_clouds = blob(model, points, offsets, poses, p)
    if program is None:
        cap = n_clouds * (56 + 128 + 696) + 4 * n_rows
        out, n = C.create_string_buffer(max(cap, 1)), C.c_uint64(0)
        rc = hostcheck_lib().hostcheck_localize(data, len(data), out, cap, C.byref(n))
        assert rc == 0 and n.value == cap, (rc, n.value, cap)
        return unpack(out.raw[:cap], n_rows, n_clouds)
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(data)
        r = subprocess.run([program, fin, fout], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        with open(fout, "rb") as f:
            return unpack(f.read(), n_rows, n_clouds)


# ---- the numpy model ---------------------------------------------------------------------------------------------------------------
NEIGHBOURS = np.array([[0, 0, 0], [-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0], [0, 0, -1], [0, 0, 1]], dtype=np.int64)


class LocalizeModel:
    """the rule on the records of a SurfelMapModel (its finish), all points of a cloud at once"""

    def __init__(self, model, p):
        self.m, self.p = model, p
        self.max_distance = model.leaf if p["max_distance"] == 0.0 else p["max_distance"]
        self.index = {}
        recs = []
        for key, e in model.vox.items():
            r = M.finish(e[0], e[1], e[2], e[3], e[4], e[5], model.leaf)
            usable = e[4] >= p["min_points"] and r[2][1] > 0.0 and r[2][0] <= p["planarity"] * r[2][1]
            self.index[key] = len(recs)
            recs.append(list(r[0]) + list(r[3]) + [1.0 if usable else 0.0])
        self.recs = np.array(recs, dtype=np.float64).reshape(len(recs), 7)

    def evaluate(self, pts, T):
        """dict(chosen (n,), near (n,) bool, H (6, 6), g (6,), cost, counters..., J, r)"""
        p = np.asarray(pts, dtype=np.float64)[:, :3]
        n = len(p)
        chosen = np.full(n, OUT_UNUSED, dtype=np.int32)
        near = np.zeros(n, dtype=bool)
        what = CM.validity(p, self.m.min_range, self.m.max_range)
        v = CM.pose_act(T, p) if n else p
        ok, cell, _ = CM.cells(v, self.m.leaf)
        live = (what == CM.USED) & ok
        J, r = [], []
        huber = self.p["huber_delta"]
        cnt = dict.fromkeys(COUNTERS, 0)
        cnt["n_unused"] = int((~live).sum())
        nk = 7 if self.p["neighborhood"] == 7 else 1
        for i in np.flatnonzero(live):
            best, d2s = None, []
            for k in range(nk):
                c = cell[i] + NEIGHBOURS[k]
                if (np.abs(c) >= CM.BIAS).any():
                    continue
                j = self.index.get(int(CM.pack(c[None])[0]))
                if j is None or not self.recs[j, 6]:
                    continue
                d = v[i] - self.recs[j, :3]
                d2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
                d2s.append(d2)
                if best is None or d2 < best[0]:
                    best = (d2, k, j)
            if best is None:
                chosen[i] = OUT_NO_SURFEL
                cnt["n_no_surfel"] += 1
                continue
            d2s.sort()
            if len(d2s) > 1 and d2s[1] - d2s[0] < NEAR:
                near[i] = True
            mean, normal = self.recs[best[2], :3], self.recs[best[2], 3:6]
            d = v[i] - mean
            s = normal[0] * d[0] + normal[1] * d[1] + normal[2] * d[2]
            if abs(abs(s) - self.max_distance) < NEAR or (huber > 0.0 and abs(abs(s) - huber) < NEAR):
                near[i] = True
            if abs(s) > self.max_distance:
                chosen[i] = OUT_GATED
                cnt["n_gated"] += 1
                continue
            g = np.copysign(1.0, s) * normal
            row = np.concatenate([np.cross(v[i], g), g])
            res = abs(s)
            if not (np.isfinite(row).all() and np.isfinite(res)):
                chosen[i] = OUT_NOT_FINITE
                cnt["n_unused"] += 1
                continue
            if huber > 0.0 and res > huber:
                sc = np.sqrt(huber / res)
                row, res = row * sc, res * sc
                cnt["n_huber"] += 1
            chosen[i] = best[1]
            cnt["n_rows"] += 1
            J.append(row), r.append(res)
        J, r = np.array(J, dtype=np.float64).reshape(len(J), 6), np.array(r, dtype=np.float64)
        out = dict(cnt, chosen=chosen, near=near, H=J.T @ J, g=J.T @ r, cost=float(r @ r), J=J, r=r)
        return out

    def solve(self, pts, T):
        """(pose, result dict, last evaluation)"""
        p = self.p
        T = np.array(T, dtype=np.float64)
        res = dict(iterations=0, termination=MAX_ITERATIONS, last_rotation=0.0, last_translation=0.0)
        first = None
        done = p["max_iterations"] == 0
        while not done:
            ev = self.evaluate(pts, T)
            first = first or ev
            if not np.isfinite(T).all():
                res["termination"] = NOT_FINITE
                break
            if ev["n_rows"] < p["min_rows"]:
                res["termination"] = TOO_FEW_ROWS
                break
            w, V = np.linalg.eigh(ev["H"])
            used = w > p["min_eigenvalue_per_row"] * ev["n_rows"]
            d = np.zeros(6)
            for i in np.flatnonzero(used):
                d -= V[:, i] * (V[:, i] @ ev["g"]) / w[i]
            q = np.array([d[0] / 2, d[1] / 2, d[2] / 2, 1.0])
            q /= np.linalg.norm(q)
            nxt = compose(np.concatenate([q, d[3:]]), T)
            if not (np.isfinite(d).all() and np.isfinite(nxt).all()):
                res["termination"] = NOT_FINITE
                break
            T = nxt
            res["iterations"] += 1
            res["last_rotation"], res["last_translation"] = float(np.linalg.norm(d[:3])), float(np.linalg.norm(d[3:]))
            if res["last_rotation"] < p["rotation_convergence_thresh"] and res["last_translation"] < p["position_convergence_thresh"]:
                res["termination"] = CONVERGED
                done = True
            elif res["iterations"] >= p["max_iterations"]:
                res["termination"] = MAX_ITERATIONS
                done = True
        ev = self.evaluate(pts, T)
        first = first or ev
        w = np.linalg.eigvalsh(ev["H"])
        res.update({k: ev[k] for k in COUNTERS})
        res.update(pose=T, initial_cost=first["cost"], final_cost=ev["cost"], n_rows_initial=first["n_rows"], eigenvalues=w,
                   used_mask=sum(1 << i for i in range(6) if w[i] > p["min_eigenvalue_per_row"] * ev["n_rows"]))
        return T, res, ev


def quat_mul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def compose(a, b):
    """a o b of two pose7"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.concatenate([quat_mul(a[:4], b[:4]), CM.pose_act(a, b[None, 4:7])[0]])


def inverse(a):
    a = np.asarray(a, dtype=np.float64)
    q = np.array([-a[0], -a[1], -a[2], a[3]]) / (a[:4] @ a[:4])
    return np.concatenate([q, -CM.pose_act(np.concatenate([q, np.zeros(3)]), a[None, 4:7])[0]])


def pose_error(a, b):
    """(metres, degrees) between two pose7 with unit quaternions"""
    d = compose(inverse(a), b)
    return float(np.linalg.norm(d[4:])), float(np.degrees(2.0 * np.arctan2(np.linalg.norm(d[:3]), abs(d[3]))))


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
H, W = 16, 256
_scene_cache = {}


def drive(name, n_scans=7):
    """(scans (n, H W, 3) sensor frame, poses (n, 7) map_T_sensor) of a short drive through an outdoor scene: the sensor moves 0.8 m
    and turns 1.2 degrees per scan"""
    if (name, n_scans) not in _scene_cache:
        boxes = S.scene_boxes(name, 0)
        o0, yaw0 = S.sensor_origin(name, 0)
        scans, poses = [], []
        for i in range(n_scans):
            yaw = yaw0 + np.radians(1.2) * i
            o = o0 + i * 0.8 * np.array([np.cos(yaw0), np.sin(yaw0), 0.0])
            scans.append(S.cast(boxes, o, yaw, H, W, S.FANS[name], 0.01, np.random.default_rng([41, i])))
            poses.append(S.yaw_pose(yaw, o))
        _scene_cache[(name, n_scans)] = (np.stack(scans), np.stack(poses))
    return _scene_cache[(name, n_scans)]


def displaced(pose, metres=0.2, degrees=1.5, seed=0):
    """`pose` moved by a fixed-seed step of that size in the sensor's own frame (so the position is off by exactly `metres`)"""
    rng = np.random.default_rng([43, seed])
    axis, t = rng.normal(size=3), rng.normal(size=3)
    axis, t = axis / np.linalg.norm(axis), t / np.linalg.norm(t) * metres
    half = np.radians(degrees) / 2
    return compose(pose, np.concatenate([np.sin(half) * axis, [np.cos(half)], t]))


_map_cache = {}


def drive_map(name, leaf=0.5, n_map=6):
    """the SurfelMapModel of the first n_map scans of the drive at their true poses (built once per process)"""
    if (name, leaf, n_map) not in _map_cache:
        scans, poses = drive(name)
        m = M.SurfelMapModel(leaf, 0.5, 120.0)
        m.recipe = (scans[:n_map].reshape(-1, 3), [i * H * W for i in range(n_map + 1)], poses[:n_map])
        m.add(m.recipe[0], offsets=m.recipe[1], poses=m.recipe[2])
        _map_cache[(name, leaf, n_map)] = m
    return _map_cache[(name, leaf, n_map)]


def floor_map(leaf=0.5, half=10.0, step=0.11):
    """a floor-only map: a grid of points on z = 0.02 seen from 1.8 m above the origin (SurfelMapModel, the points in the map frame)"""
    g = np.arange(-half, half, step)
    x, y = np.meshgrid(g, g)
    rng = np.random.default_rng(47)
    pts = np.stack([x.ravel(), y.ravel(), 0.02 + 0.002 * rng.standard_normal(x.size)], axis=1)
    pose = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.8])
    m = M.SurfelMapModel(leaf, 0.5, 120.0)
    m.recipe = (pts - pose[4:], [0, len(pts)], pose[None])
    m.add(m.recipe[0], poses=m.recipe[2])
    return m, pts - pose[4:], pose


# ---- the candidate and gate cases: {name: (model, points (n, 3), pose7, params, expected outcome per point)} ---------------------------
IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
_SYM = (8192, 24576, 40960, 57344)  # offsets inside a voxel whose mean is exactly half an edge


def _patch(corner, axis, at=32768, leaf=1.0):
    """16 lattice points of voxel `corner` on the plane (coordinate `axis`) = corner + at / 65536: its mean lies exactly in the middle
    of the other two axes, its normal is exactly the axis"""
    a, b = [k for k in range(3) if k != axis]
    steps = np.zeros((16, 3), dtype=np.int64)
    steps[:, axis] = at
    steps[:, a], steps[:, b] = np.repeat(_SYM, 4), np.tile(_SYM, 4)
    return (np.asarray(corner, dtype=np.float64) + steps / M.UNIT) * leaf


def _micro_map(*clouds, max_range=120.0):
    m = M.SurfelMapModel(1.0, 0.0, max_range)
    m.recipe = (np.concatenate(clouds), [0, sum(len(c) for c in clouds)], None)  # (points, offsets, poses): how a device map gets the same voxels
    m.add(m.recipe[0])
    return m


def micro_cases():
    """every case is one evaluation (max_iterations = 0) at the identity pose of a map made by hand at leaf 1.0"""
    cases = {}
    ev = dict(max_iterations=0, min_rows=0)
    wall = _patch((5, 5, 5), 0, at=58982)  # the plane x = 5.9
    q = np.array([[6.1, 5.5, 5.5]])
    cases["home_empty_neighbour_usable_7"] = (_micro_map(wall), q, IDENTITY, params(**ev), [1])
    cases["home_empty_neighbour_usable_1"] = (_micro_map(wall), q, IDENTITY, params(neighborhood=1, **ev), [OUT_NO_SURFEL])
    few = _patch((6, 5, 5), 2)[:3]  # three points: below min_points = 5
    cases["home_below_min_points_7"] = (_micro_map(wall, few), q, IDENTITY, params(**ev), [1])
    cases["home_below_min_points_1"] = (_micro_map(wall, few), q, IDENTITY, params(neighborhood=1, **ev), [OUT_NO_SURFEL])
    cases["home_at_min_points_3"] = (_micro_map(wall, few), q, IDENTITY, params(min_points=3, planarity=1.0, **ev), None)
    cube = (np.array([6.0, 5.0, 5.0]) + np.array([[x, y, z] for x in _SYM[::3] for y in _SYM[::3] for z in _SYM[::3]]) / M.UNIT)
    cases["home_a_cube_lattice"] = (_micro_map(wall, cube), q, IDENTITY, params(**ev), [1])
    line = np.array([6.0, 5.0, 5.0]) + np.stack([np.arange(8) * 8000 + 500, np.full(8, 30000), np.full(8, 30000)], axis=1) / M.UNIT
    cases["home_a_line_along_x"] = (_micro_map(wall, line), q, IDENTITY, params(**ev), [1])
    diag = np.array([6.0, 5.0, 5.0]) + np.stack([np.arange(8) * 8000 + 500] * 3, axis=1) / M.UNIT
    cases["home_a_diagonal_line"] = (_micro_map(wall, diag), q, IDENTITY, params(**ev), None)
    # two candidates at exactly the same distance: -x comes before +x
    left, right = _patch((5, 5, 5), 2), _patch((7, 5, 5), 2)
    cases["tie_minus_x_before_plus_x"] = (_micro_map(left, right), np.array([[6.5, 5.5, 5.625]]), IDENTITY, params(**ev), [1])
    cases["tie_minus_y_before_plus_z"] = (_micro_map(_patch((6, 4, 5), 0), _patch((6, 5, 6), 0)), np.array([[6.5, 5.5, 5.5]]), IDENTITY,
                                          params(**ev), [3])
    # the face neighbour beyond |v| = 2^20 is skipped, on both sides
    far = 1048575.0
    cases["neighbour_across_plus_2_20"] = (_micro_map(_patch((far - 1, 5, 5), 2), max_range=2e6), np.array([[far + 0.5, 5.5, 5.625]]), IDENTITY,
                                           params(**ev), [1])
    cases["neighbour_across_minus_2_20"] = (_micro_map(_patch((-far + 1, 5, 5), 2), max_range=2e6), np.array([[-far + 0.5, 5.5, 5.625]]),
                                            IDENTITY, params(**ev), [2])
    # |s| exactly at max_distance / huber_delta, and one unit in the last place beyond
    floor = _patch((5, 5, 5), 2)  # z = 5.5 exactly
    up = np.nextafter(5.75, 6.0)
    pts = np.array([[5.5, 5.5, 5.75], [5.5, 5.5, up], [5.5, 5.5, 5.25], [5.5, 5.5, np.nextafter(5.25, 5.0)]])
    cases["s_at_max_distance"] = (_micro_map(floor), pts, IDENTITY, params(max_distance=0.25, huber_delta=0.0, **ev), [0, OUT_GATED, 0, OUT_GATED])
    cases["s_at_huber_delta"] = (_micro_map(floor), pts, IDENTITY, params(huber_delta=0.25, **ev), [0, 0, 0, 0])
    cases["huber_off"] = (_micro_map(floor), pts, IDENTITY, params(huber_delta=0.0, **ev), [0, 0, 0, 0])
    return cases


def information_from_records(rec, dist, v, p, leaf):
    """sum J^T J and the row count at neighbourhood 1 from the records and distances a surfel map's query gives for the moved points v
    (its min_points = p's): the usable test, the gate and Huber in numpy"""
    usable = (rec["count"] >= max(p["min_points"], 1)) & (rec["eval"][:, 1] > 0.0) & (rec["eval"][:, 0] <= p["planarity"] * rec["eval"][:, 1])
    gate = leaf if p["max_distance"] == 0.0 else p["max_distance"]
    keep = usable & (np.abs(dist) <= gate)
    g = np.copysign(1.0, dist[keep])[:, None] * rec["normal"][keep]
    J = np.concatenate([np.cross(v[keep], g), g], axis=1)
    r = np.abs(dist[keep])
    if p["huber_delta"] > 0.0:
        sc = np.where(r > p["huber_delta"], np.sqrt(p["huber_delta"] / np.maximum(r, 1e-300)), 1.0)
        J = J * sc[:, None]
    return J.T @ J, int(keep.sum())
