"""The rule of the occupancy map (include/loamx.h, "occupancy map") in plain numpy: validity, end points, hit voxel, the voxel
walk and the state of a voxel, float64 operations one at a time in the header's order (numpy's elementwise loops round every
operation on its own), so everything is compared by equality. Vectorised over rays, a Python loop over the steps of the walk.
The map itself is a dict voxel key -> [hits, passes]. No code shared with the kernels; the pose transform, the voxel of a point
and the key packing are those of tests/cloudmap_common.py. Also: the binding of tests/hostcheck_occupancy."""
import ctypes as C
import os
import subprocess

import numpy as np

import cloudmap_common as CM

BIAS = CM.BIAS
UNKNOWN, FREE, OCCUPIED = 0, 1, 2
NORMAL, INVALID, SHORT, LONG = range(4)
STAT_NAMES = ("rays_offered", "rays_hit", "invalid", "range_short", "range_long", "outside", "visits", "voxels", "overflow")
DEFAULTS = dict(leaf=0.2, min_range=0.5, max_range=80.0, end_margin=0.2, clip_long=1, min_hits=1, occ_ratio=0.0, min_passes=1)
same_bytes = CM.same_bytes


def classify(p, min_range, max_range):
    """(kind, r2) per point (step 1); p: (n, 3) float64"""
    with np.errstate(all="ignore"):
        r2 = p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2]
        finite = np.isfinite(p).all(axis=1) & np.isfinite(r2)
        kind = np.where(~finite, INVALID, np.where(~(r2 >= min_range * min_range), SHORT, np.where(~(r2 <= max_range * max_range), LONG, NORMAL)))
    return kind, r2


class Rays:
    """steps 1 to 4 of n rays of one cloud up to the first voxel of their walks"""

    def __init__(self, points, pose, leaf, min_range, max_range, end_margin, clip_long):
        p = np.asarray(points)[:, :3].astype(np.float64)
        n = len(p)
        self.n = n
        self.kind, r2 = classify(p, min_range, max_range)
        is_long = self.kind == LONG
        alive = (self.kind == NORMAL) | (is_long & bool(clip_long))
        with np.errstate(all="ignore"):
            if pose is None:
                q, o = p, np.zeros(3)
            else:
                pose = np.asarray(pose, dtype=np.float64)
                q, o = CM.pose_act(pose, p), pose[4:7]
            d = q - o
            dist = np.sqrt(r2)
            s = np.where(is_long, max_range / dist, (dist - end_margin) / dist)
            e = o + s[:, None] * d
            cell_ok, hv, _ = CM.cells(q, leaf)
            normal = alive & ~is_long
            self.has_hit = normal & cell_ok
            self.hit_key = np.where(self.has_hit, CM.pack(hv), np.uint64(0))
            dropped_whole = normal & ~cell_ok
            wants_walk = alive & ~dropped_whole & (s > 0.0)
            to, te = np.broadcast_to(o / leaf, (n, 3)), e / leaf
            v, ve = np.floor(to), np.floor(te)
            in_range = np.all(np.abs(v) < BIAS, axis=1) & np.all(np.abs(ve) < BIAS, axis=1)
            self.walks = wants_walk & in_range
            self.outside = dropped_whole | (wants_walk & ~in_range)
            w = self.walks[:, None]
            v, ve = np.where(w, v, 0.0), np.where(w, ve, 0.0)
            self.v, self.ve = v.astype(np.int64), ve.astype(np.int64)
            self.dir = np.where(self.ve >= self.v, 1, -1)
            self.rem = np.abs(self.ve - self.v)
            ad = np.abs(te - to)
            stepping = w & (self.rem > 0)
            self.t_delta = np.where(stepping, 1.0 / ad, 0.0)
            self.t_max = np.where(stepping, np.where(self.dir > 0, (v + 1.0) - to, to - v) / ad, 0.0)
        self.steps = np.where(self.walks, self.rem.sum(axis=1), 0)

    def visits(self):
        """yields per step (standing, keys): the rays that stand in a voxel of their walk in this step and that voxel's key
        (0 elsewhere); the first step is the start voxel. Every visit of a ray, its own hit voxel included."""
        v, rem, t_max = self.v.copy(), self.rem.copy(), self.t_max.copy()
        left = np.where(self.walks, self.steps + 1, 0)
        rows = np.arange(self.n)
        while (left > 0).any():
            standing = left > 0
            yield standing, np.where(standing, CM.pack(v), np.uint64(0))
            left = left - standing
            go = left > 0
            pick = np.argmin(np.where(rem > 0, t_max, np.inf), axis=1)  # (the first of equal minima: ties go to the lowest axis)
            r, a = rows[go], pick[go]
            assert (rem[r, a] > 0).all()
            v[r, a] += self.dir[r, a]
            t_max[r, a] = t_max[r, a] + self.t_delta[r, a]
            rem[r, a] -= 1
        self.end = v  # (where the walks stopped: the tests compare it with ve)

    def visit_lists(self):
        """per ray the keys of its walk in order (an empty list for a ray without a walk)"""
        out = [[] for _ in range(self.n)]
        for standing, keys in self.visits():
            for i in np.flatnonzero(standing):
                out[i].append(int(keys[i]))
        return out


def state(hits, passes, min_hits=1, occ_ratio=0.0, min_passes=1):
    """step 5 on arrays of counts"""
    hits, passes = np.asarray(hits, dtype=np.uint32), np.asarray(passes, dtype=np.uint32)
    occupied = (hits >= min_hits) & (hits.astype(np.float64) >= occ_ratio * passes.astype(np.float64))
    return np.where(occupied, OCCUPIED, np.where(passes >= min_passes, FREE, UNKNOWN)).astype(np.uint8)


def key_coords(keys):
    keys = np.asarray(keys, dtype=np.uint64)
    m = np.uint64(0x1FFFFF)
    return np.stack([((keys >> np.uint64(s)) & m).astype(np.int64) - BIAS for s in (42, 21, 0)], axis=-1)


class OccupancyModel:
    def __init__(self, **params):
        self.p = dict(DEFAULTS, **params)
        self.clear()

    def clear(self):
        self._vox = {}  # key -> [hits, passes]
        self._pending = ([], [])  # key arrays of hits and of passes that the dict has not taken yet
        self.st = dict.fromkeys(STAT_NAMES, 0)
        self.wave_claims = self.plain_claims = 0

    def _bump(self, keys, which):
        self._pending[which].append(keys)

    @property
    def vox(self):
        for which, arrays in enumerate(self._pending):
            if arrays:
                ks, counts = np.unique(np.concatenate(arrays), return_counts=True)
                for k, c in zip(ks.tolist(), counts.tolist()):
                    self._vox.setdefault(k, [0, 0])[which] += c
                arrays.clear()
        return self._vox

    def add(self, points, offsets=None, poses=None):
        """points: (n, k >= 3) float64 or float32; offsets: n_clouds + 1 point offsets (None: one cloud); poses: (n_clouds, 7) or
        None. wave_claims counts what the run-combining kernel claims: per wavefront (64 consecutive rays of a launch; a call is one
        launch per 256 clouds, of fewer than 2^30 rays each) and step, the runs of neighbouring lanes with a visit and the same key."""
        pts = np.asarray(points)
        offsets = [0, len(pts)] if offsets is None else [int(o) for o in offsets]
        p = self.p
        clouds = [Rays(pts[offsets[c]:offsets[c + 1]], None if poses is None else poses[c], p["leaf"], p["min_range"], p["max_range"],
                       p["end_margin"], p["clip_long"]) for c in range(len(offsets) - 1)]
        st = self.st
        st["rays_offered"] += offsets[-1] - offsets[0]
        if not clouds or offsets[-1] == offsets[0]:
            return
        cat = lambda name: np.concatenate([getattr(r, name) for r in clouds])
        kind, has_hit, hit_key = cat("kind"), cat("has_hit"), cat("hit_key")
        st["invalid"] += int((kind == INVALID).sum())
        st["range_short"] += int((kind == SHORT).sum())
        st["range_long"] += int((kind == LONG).sum())
        st["outside"] += int(cat("outside").sum())
        st["rays_hit"] += int(has_hit.sum())
        self._bump(hit_key[has_hit], 0)
        self.plain_claims += int(has_hit.sum())
        # a call is one launch per 256 clouds: the wavefronts of a launch are counted from its first ray
        starts = [offsets[c] - offsets[0] for c in range(0, len(clouds), 256)] + [offsets[-1] - offsets[0]]
        launches = [slice(a, b) for a, b in zip(starts[:-1], starts[1:]) if b > a]
        wave_runs = lambda on, key: sum(CM.wave_runs(on[l], key[l]) for l in launches)
        self.wave_claims += wave_runs(has_hit, hit_key)
        walkers = [r.visits() for r in clouds]
        while True:
            parts = [next(w, None) for w in walkers]
            if all(x is None for x in parts):
                break
            standing = np.concatenate([np.zeros(r.n, dtype=bool) if x is None else x[0] for r, x in zip(clouds, parts)])
            keys = np.concatenate([np.zeros(r.n, dtype=np.uint64) if x is None else x[1] for r, x in zip(clouds, parts)])
            on = standing & ~(has_hit & (keys == hit_key))
            st["visits"] += int(on.sum())
            self._bump(keys[on], 1)
            self.plain_claims += int(on.sum())
            self.wave_claims += wave_runs(on, keys)
        st["voxels"] = len(self.vox)

    def stats(self):
        return dict(self.st)

    def _state(self, counts):
        return state(counts[..., 0], counts[..., 1], self.p["min_hits"], self.p["occ_ratio"], self.p["min_passes"])

    def query(self, points):
        """(counts (n, 2) uint32, state (n,) uint8)"""
        pts = np.asarray(points, dtype=np.float64)[:, :3]
        ok, v, _ = CM.cells(pts, self.p["leaf"])
        keys = CM.pack(v)
        counts = np.array([self.vox.get(int(k), [0, 0]) if o else [0, 0] for k, o in zip(keys, ok)], dtype=np.uint32).reshape(-1, 2)
        return counts, self._state(counts)

    def box(self, vmin, dims):
        """(counts (dz, dy, dx, 2) uint32, state (dz, dy, dx) uint8): x fastest"""
        vmin, dims = np.asarray(vmin, dtype=np.int64), np.asarray(dims, dtype=np.int64)
        counts = np.zeros((dims[2], dims[1], dims[0], 2), dtype=np.uint32)
        if self.vox and counts.size:
            c = key_coords(list(self.vox)) - vmin
            inside = np.all((c >= 0) & (c < dims), axis=1)
            vals = np.array(list(self.vox.values()), dtype=np.uint32)
            counts[c[inside, 2], c[inside, 1], c[inside, 0]] = vals[inside]
        return counts, self._state(counts)

    def slice(self, vmin, dims):
        """(dy, dx) uint8: per column the largest state of its levels (OCCUPIED > FREE > UNKNOWN)"""
        s = self.box(vmin, dims)[1]
        return s.max(axis=0) if s.shape[0] else np.zeros(s.shape[1:], dtype=np.uint8)

    def bounds(self, pad=1):
        """(vmin, dims) of a box around every voxel of the map"""
        c = key_coords(list(self.vox))
        lo, hi = c.min(axis=0) - pad, c.max(axis=0) + pad
        return lo.astype(np.int32), (hi - lo + 1).astype(np.uint32)


def assert_stats_equal(got, want, what=""):
    g = {n: int(got[n]) for n in STAT_NAMES}
    assert g == {n: int(want[n]) for n in STAT_NAMES}, (what, g, want)


# ---- tests/hostcheck_occupancy: occupancy_math.h compiled by g++ -----------------------------------------------------------------
HOSTCHECK_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck_occupancy")
_lib = None


def hostcheck_lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", HOSTCHECK_DIR])
        _lib = C.CDLL(os.path.join(HOSTCHECK_DIR, "libhostcheck_occupancy.so"))
    return _lib


# ---- the rays both the g++ build and the kernels are compared on ---------------------------------------------------------------------
def _pose(t=(0.0, 0.0, 0.0), yaw=0.0):
    return np.array([0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2), *t], dtype=np.float64)


WALK_END_CASES = {}  # filled by walk_cases: name -> (the ray lost or None, the coordinate ve of the ray that reaches furthest)


def walk_cases():
    """name -> (params, points (n, 3), pose7 or None): the edges of the rule, one cloud each"""
    up, dn = (lambda x: np.nextafter(x, np.inf)), (lambda x: np.nextafter(x, -np.inf))
    a = np.array([0.5, 1.0, 1.5, 2.0, 3.25, 7.5, 20.0])
    diag = np.concatenate([np.stack([a, a, 0 * a], 1), np.stack([a, a, a], 1), np.stack([-a, -a, a], 1)])
    axes = np.concatenate([np.stack([s * a if k == j else 0 * a for k in range(3)], 1) for j in range(3) for s in (1, -1)])
    big = float(BIAS)
    cases = {}
    for leaf in (0.5, 0.2):
        for margin in (0.0, 0.25):
            p = dict(leaf=leaf, min_range=0.3, max_range=60.0, end_margin=margin)
            cases[f"corner_diagonals_{leaf}_{margin}"] = (p, diag, _pose((2 * leaf, -3 * leaf, leaf)))
            cases[f"axis_parallel_{leaf}_{margin}"] = (p, axes, _pose((0.3 * leaf, -0.6 * leaf, 0.5 * leaf)))
    cases["corner_diagonals_no_pose"] = (dict(leaf=0.5, min_range=0.3, end_margin=0.0), diag, None)
    tiny = np.array([[0.05, 0.03, 0.02], [0.11, -0.01, 0.04], [0.02, 0.02, -0.02], [0.2, 0.1, 0.1]])
    cases["inside_one_voxel"] = (dict(leaf=0.5, min_range=0.01, end_margin=0.0), tiny, _pose((0.2, 0.2, 0.2)))
    faces = np.array([[1.5, -1.0, 0.5], [-2.0, -2.0, -2.0], [0.5, 0.0, 0.0], [0.0, -0.5, 0.0], [-0.0, -0.0, 1.0], [3.0, 1e-20, -1e-20],
                      [-1e-20, -1.5, 1e-20], [-0.75, -1.25, -3.5]])
    for name, t in (("plus_zero", (0.0, 0.0, 0.0)), ("minus_zero", (-0.0, -0.0, -0.0)), ("minus_tiny", (-1e-20, -1e-20, -1e-20)),
                    ("negative", (-4.3, -0.7, -2.0)), ("on_a_face", (-1.5, 2.0, -0.5))):
        cases[f"faces_origin_{name}"] = (dict(leaf=0.5, min_range=0.3, end_margin=0.0), faces, _pose(t))
    m = 0.25
    near = np.array([[m, 0, 0], [dn(m), 0, 0], [up(m), 0, 0], [0, -m, 0], [0, 0, dn(m)], [0, up(m), 0], [0.2, 0, 0], [dn(0.2), 0, 0], [0.3, 0.1, 0.0]])
    cases["the_end_margin_edge"] = (dict(leaf=0.1, min_range=0.01, end_margin=m), near, _pose((0.03, 0.04, 0.05), 0.4))
    cases["the_end_margin_edge_02"] = (dict(leaf=0.1, min_range=0.01, end_margin=0.2), near, None)
    lo, hi = 0.5, 10.0
    edges = np.array([[lo, 0, 0], [dn(lo), 0, 0], [up(lo), 0, 0], [0, hi, 0], [0, dn(hi), 0], [0, up(hi), 0], [0, 0, 0], [12.0, 1.0, 0.5],
                      [-30.0, 40.0, 2.0], [1e200, 0, 0], [1e150, 1e150, 0], [np.nan, 0, 0], [0, np.inf, 0], [1, 1, -np.inf], [0, 0, 0], [3.0, 4.0, 0.0]])
    for clip in (1, 0):
        cases[f"ranges_long_rays_and_bad_points_clip_{clip}"] = (dict(leaf=0.2, min_range=lo, max_range=hi, clip_long=clip), edges, _pose((1.0, -2.0, 0.3), 1.1))
    # |v| = 2^20 - 1 and 2^20: the hit (rays 0, 1), the origin (two poses), the end of a long ray's walk (two max_range)
    L = 0.5
    reach = np.array([[1.75 * L, 0, 0], [2.75 * L, 0, 0], [-2.0 * L, 0.3, 0], [3000.0, 0, 0], [0, 3000.0, 0]])
    for name, tx, max_range in (("origin_inside", (big - 2.5) * L, 2.0), ("long_ray_ends_on_the_last_voxel", (big - 2.5) * L, 0.75),
                                ("origin_outside", (big + 0.25) * L, 2.0), ("origin_at_minus_2_20", -big * L, 2.0),
                                ("origin_at_minus_2_20_plus_1", -(big - 1) * L, 2.0)):
        cases[f"voxel_range_{name}"] = (dict(leaf=L, min_range=0.5, max_range=max_range, end_margin=0.0), reach, _pose((tx, 0.0, 0.0)))
        cases[f"voxel_range_y_{name}"] = (dict(leaf=L, min_range=0.5, max_range=max_range, end_margin=0.0), reach[:, [1, 0, 2]], _pose((0.0, tx, 0.0)))
    # ... and the walk end where it ALONE decides: long rays (no hit) from an origin well inside, ray 0 along +a and ray 1 along -a.
    # WALK_END_CASES: name -> the one ray that is counted outside and does not walk (None: every ray walks)
    beams = np.array([[3000.0, 0, 0], [-3000.0, 0, 0], [0, 3000.0, 0]])
    for name, sign, max_range, lost in (("at_2_20", 1, 1.5, 0), ("at_2_20_minus_1", 1, 1.0, None), ("at_minus_2_20", -1, 1.0, 1),
                                        ("at_minus_2_20_plus_1", -1, 0.5, None)):
        p = dict(leaf=L, min_range=0.5, max_range=max_range, end_margin=0.0)
        cases[f"voxel_range_walk_end_{name}"] = (p, beams, _pose((sign * (big - 2.5) * L, 0.0, 0.0)))
        cases[f"voxel_range_walk_end_y_{name}"] = (p, beams[:, [1, 0, 2]], _pose((0.0, sign * (big - 2.5) * L, 0.0)))
        WALK_END_CASES[f"voxel_range_walk_end_{name}"] = WALK_END_CASES[f"voxel_range_walk_end_y_{name}"] = (lost, sign * (BIAS if lost is not None else BIAS - 1))
    return cases


def random_rays(seed=5, n=3000, reach=90.0):
    """(points, pose): rays of every length up to `reach` (the default: beyond the default max_range) at a rotated, translated pose"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3)) * [1.0, 1.0, 0.3]
    d /= np.linalg.norm(d, axis=1)[:, None]
    pts = d * rng.uniform(0.2, reach, (n, 1))
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return pts, np.concatenate([q, rng.uniform(-20, 20, 3)])
