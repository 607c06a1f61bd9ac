"""The rule of the occupancy ray cast (include/loamx.h, "occupancy ray casting") in plain Python: scalar float64 operations one at
a time in the order of loam_amd/csrc/raycast_math.h (a Python float is an IEEE double and every operator rounds on its own), so
everything is compared by equality, t_enter and t_exit as bit patterns. The states of the voxels come from the model of the map
in tests/occupancy_common.py (or from any dict key -> (hits, passes)). No code shared with the kernels; the pose transform is
that of tests/cloudmap_common.py. Also: the case lists of the tests and the binding of tests/hostcheck_raycast."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import cloudmap_common as CM
import occupancy_common as OM

BIAS = CM.BIAS
CLEAR, HIT, UNKNOWN, TRUNCATED, OUTSIDE, INVALID = range(6)
STATUS_NAMES = ("clear", "hit", "unknown", "truncated", "outside", "invalid")
AT_ENTER, AT_MIDDLE = 0, 1
DEFAULT_MAX_STEPS = 3 * 4098
MAX_STEPS_LIMIT = 1 << 22
DEFAULTS = dict(skip_start=0, unknown_stops=0, max_steps=DEFAULT_MAX_STEPS, hit_at=AT_MIDDLE)
CENSUS_NAMES = ("rays", "visits", "probes", "hit", "unknown", "clear", "truncated", "outside", "invalid")
RECORD_DTYPE = np.dtype([("status", "<u4"), ("visits", "<u4"), ("voxel", "<i4", (3,)), ("n_unknown", "<u4"), ("t_enter", "<f8"), ("t_exit", "<f8")])
assert RECORD_DTYPE.itemsize == 40
same_bytes = CM.same_bytes


def pack(b):
    return (b[0] << 42) | (b[1] << 21) | b[2]


def _finite(v):
    return v - v == 0.0


class Walk:
    """occ_walk_begin: None (through begin()) where a voxel coordinate is outside |v| < 2^20"""

    @staticmethod
    def begin(o, e, leaf):
        w = Walk()
        w.b, w.rem, w.dir, w.t_max, w.t_delta = [0] * 3, [0] * 3, [1] * 3, [0.0] * 3, [0.0] * 3
        ok = True
        for a in range(3):
            to, te = o[a] / leaf, e[a] / leaf
            fv, fve = float(np.floor(to)), float(np.floor(te))  # (floor(-0.0) is -0.0, and to - v below sees the sign)
            if not (abs(fv) < BIAS) or not (abs(fve) < BIAS):
                ok = False
                continue
            v, ve = int(fv), int(fve)
            w.b[a] = v + BIAS
            w.dir[a] = 1 if ve >= v else -1
            w.rem[a] = abs(ve - v)
            if w.rem[a] > 0:
                ad = abs(te - to)
                w.t_delta[a] = 1.0 / ad
                w.t_max[a] = (((fv + 1.0) - to) if w.dir[a] > 0 else (to - fv)) / ad
        return w if ok else None

    def steps(self):
        return sum(self.rem)

    def step(self):
        """ray_walk_step: the picked t_max before it is advanced"""
        pick, best = -1, 0.0
        for a in range(3):
            if self.rem[a] > 0 and (pick < 0 or self.t_max[a] < best):
                pick, best = a, self.t_max[a]
        self.b[pick] += self.dir[pick]
        self.t_max[pick] = self.t_max[pick] + self.t_delta[pick]
        self.rem[pick] -= 1
        return best

    def t_exit(self):
        live = [self.t_max[a] for a in range(3) if self.rem[a] > 0]
        return min(live) if live else 1.0


class StateMap:
    """key -> state under one state rule, from a dict key -> (hits, passes)"""

    def __init__(self, vox, min_hits=1, occ_ratio=0.0, min_passes=1):
        keys = list(vox)
        counts = np.array([vox[k] for k in keys], dtype=np.uint32).reshape(-1, 2)
        self.rule = (min_hits, occ_ratio, min_passes)
        self.none = int(OM.state([0], [0], *self.rule)[0])
        self.states = dict(zip(keys, OM.state(counts[:, 0], counts[:, 1], *self.rule).tolist()))

    @staticmethod
    def of(model):
        return StateMap(model.vox, model.p["min_hits"], model.p["occ_ratio"], model.p["min_passes"])

    def __call__(self, key):
        return self.states.get(key, self.none)


def zero_record(status):
    return (status, 0, (0, 0, 0), 0, 0.0, 0.0)


def cast_one(o, e, leaf, states, P, trace=None):
    """one ray: the record as a tuple in RECORD_DTYPE's order; trace (a list) takes (key, tested, t_enter, t_exit) per visit"""
    if not all(_finite(float(c)) for c in (*o, *e)):
        return zero_record(INVALID)
    w = Walk.begin([float(c) for c in o], [float(c) for c in e], leaf)
    if w is None:
        return zero_record(OUTSIDE)
    left, cap, visits, n_unknown, t_enter = w.steps(), P["max_steps"], 0, 0, 0.0
    while True:
        tested = visits >= P["skip_start"]
        if trace is not None:
            trace.append((pack(w.b), tested, t_enter, w.t_exit()))
        visits += 1
        status = None
        if tested:
            st = states(pack(w.b))
            if st == OM.OCCUPIED:
                status = HIT
            elif st == OM.UNKNOWN:
                if P["unknown_stops"]:
                    status = UNKNOWN
                else:
                    n_unknown += 1
        if status is None:
            if left == 0:
                status = CLEAR
            elif cap == 0:
                status = TRUNCATED
        if status is not None:
            return (status, visits, tuple(b - BIAS for b in w.b), n_unknown, t_enter, w.t_exit())
        t_enter = w.step()
        left, cap = left - 1, cap - 1


def wave_probes(traces):
    """the look-ups of the combining form for the rays of one call in input order: per wavefront (64 consecutive rays) and trip, a
    lane that tests its voxel opens a run unless the lane before it is in the same wavefront, tests too and holds the same key"""
    probes = 0
    for w0 in range(0, len(traces), 64):
        wave = traces[w0:w0 + 64]
        for k in range(max((len(t) for t in wave), default=0)):
            before = None
            for t in wave:
                now = t[k][0] if k < len(t) and t[k][1] else None
                probes += now is not None and now != before
                before = now
    return probes


def cast(origins, ends, leaf, states, params=None):
    """(records, census): the model of loamx_occupancy_cast_rays; census["probes"] is a pair (plain, combined)"""
    P = dict(DEFAULTS, **(params or {}))
    origins, ends = np.asarray(origins, dtype=np.float64).reshape(-1, 3), np.asarray(ends, dtype=np.float64).reshape(-1, 3)
    traces = [[] for _ in origins]
    recs = [cast_one(o.tolist(), e.tolist(), leaf, states, P, tr) for o, e, tr in zip(origins, ends, traces)]
    return to_records(recs), census_of(recs, traces)


def to_records(recs):
    out = np.zeros(len(recs), dtype=RECORD_DTYPE)
    for i, r in enumerate(recs):
        out[i] = r
    return out


def census_of(recs, traces):
    tested = sum(sum(1 for v in t if v[1]) for t in traces)
    c = dict(rays=len(recs), visits=tested, probes=(tested, wave_probes(traces)))
    for s, name in enumerate(STATUS_NAMES):
        c[name] = sum(1 for r in recs if r[0] == s)
    return c


def render(dirs, poses, max_range, leaf, states, params=None):
    """(scans (n_poses, n_beams, 3), ranges, records, census): the model of loamx_occupancy_render_scans"""
    P = dict(DEFAULTS, **(params or {}))
    dirs, poses = np.asarray(dirs, dtype=np.float64).reshape(-1, 3), np.asarray(poses, dtype=np.float64).reshape(-1, 7)
    recs, traces, scans, ranges = [], [], [], []
    for pose in poses:
        ok = bool(np.isfinite(pose).all())
        far = np.stack([max_range * dirs[:, 0], max_range * dirs[:, 1], max_range * dirs[:, 2]], axis=1)
        ends = CM.pose_act(pose, far) if ok else None
        for b, d in enumerate(dirs.tolist()):
            tr = []
            r = cast_one(pose[4:7].tolist(), ends[b].tolist(), leaf, states, P, tr) if ok else zero_record(INVALID)
            rng, p = 0.0, (0.0, 0.0, 0.0)
            if r[0] == HIT:
                tau = r[4] if P["hit_at"] == AT_ENTER else 0.5 * (r[4] + r[5])
                rng = tau * max_range
                p = (rng * d[0], rng * d[1], rng * d[2])
            recs.append(r), traces.append(tr), scans.append(p), ranges.append(rng)
    shape = (len(poses), len(dirs))
    return (np.array(scans, dtype=np.float64).reshape(*shape, 3), np.array(ranges, dtype=np.float64).reshape(shape),
            to_records(recs).reshape(shape), census_of(recs, traces))


def assert_census(got, want, combined, what=""):
    want = dict(want, probes=want["probes"][1 if combined else 0])
    g = {n: int(got[n]) for n in CENSUS_NAMES}
    assert g == {n: int(want[n]) for n in CENSUS_NAMES}, (what, g, want)


# ---- the hand-made map and the rays both the g++ build and the kernels are compared on -------------------------------------------
LEAF = 0.5
HAND_PARAMS = dict(leaf=LEAF, min_range=0.1, max_range=30.0, end_margin=0.0)
HAND_POSE = np.array([0.0, 0.0, 0.0, 1.0, 0.25, 0.25, 0.25])
HAND_MAX_VOXELS = 64  # 128 slots for the voxels below: probe chains occur


def hand_cloud():
    """one cloud seen from the centre of voxel (0, 0, 0): a wall of 5 x 2 voxels at x = 8 (y -2 .. 2, z 0 .. 1) and a lone voxel
    (-6, 0, 0); everything between the sensor and them is FREE, everything else nobody saw"""
    wall = [(4.0, 0.5 * j, 0.5 * k) for j in range(-2, 3) for k in range(2)]
    return np.array(wall + [(-3.0, 0.0, 0.0)], dtype=np.float64)


def hand_model():
    m = OM.OccupancyModel(**HAND_PARAMS)
    m.add(hand_cloud(), poses=HAND_POSE[None])
    assert 40 < len(m.vox) < 100 and m.stats()["rays_hit"] == 11
    return m


C0 = (0.25, 0.25, 0.25)  # the centre of voxel (0, 0, 0)
STEPS_OF_THE_CAPPED_RAY = 9


def ray_cases():
    """name -> (origins (n, 3), ends (n, 3)) on the hand-made map"""
    c = np.array(C0)
    big = float(BIAS) * LEAF
    cases = {}
    cases["o_equals_e"] = ([C0, (4.25, 0.25, 0.25), (0.25, 9.25, 0.25)], [C0, (4.25, 0.25, 0.25), (0.25, 9.25, 0.25)])
    axes = [tuple(s * 6.0 if k == a else 0.0 for k in range(3)) for a in range(3) for s in (1, -1)]
    cases["along_an_axis"] = ([C0] * 6, [tuple(c + np.array(d)) for d in axes])
    cases["lattice_corner_diagonals"] = ([(0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 0.5), (1.0, 1.0, 0.5)],
                                         [(3.0, 3.0, 3.0), (-3.0, -3.0, -3.0), (3.0, 3.0, 2.5), (-2.0, -2.0, -2.5)])
    cases["hit_in_visit_0"] = ([(4.25, 0.25, 0.25), (4.4, 0.3, 0.7)], [C0, (2.0, 1.0, 0.25)])
    cases["hit_in_the_last_voxel"] = ([C0, C0], [(4.25, 0.25, 0.25), (4.49, 1.2, 0.6)])
    cases["one_voxel_short_of_the_wall"] = ([C0, C0], [(3.75, 0.25, 0.25), (3.99, 1.2, 0.6)])
    cases["through_a_gap_nobody_saw"] = ([(6.25, 0.25, 0.25), C0, (2.25, 4.25, 0.25)], [C0, (0.25, 5.25, 0.25), (4.25, 1.25, 0.25)])
    cases["the_capped_ray"] = ([C0], [(3.75, 1.25, 0.25)])
    cases["beyond_the_voxel_range"] = ([C0, (big + 1.0, 0.0, 0.0), C0], [(big + 1.0, 0.25, 0.25), C0, (0.25, -big - 0.25, 0.25)])
    cases["not_finite"] = ([(np.nan, 0.0, 0.0), C0, C0, (0.0, -np.inf, 0.0)], [C0, (1.0, np.inf, 0.0), (1.0, 2.0, np.nan), C0])
    cases["one_run"] = ([C0] * 64, [(3.75, 1.25, 0.25)] * 64)
    cases["alternating_abab"] = ([C0, (0.25, 0.75, 0.25)] * 32, [(3.75, 0.25, 0.25), (3.75, 0.75, 0.25)] * 32)
    # even lanes end after two voxels, their odd neighbours go on through the same voxels: a run must not bridge a finished lane
    cases["short_even_lanes"] = ([C0] * 64, [(0.75, 0.25, 0.25), (3.75, 0.25, 0.25)] * 32)
    out = {}
    for name, (o, e) in cases.items():
        out[name] = (np.array(o, dtype=np.float64).reshape(-1, 3), np.array(e, dtype=np.float64).reshape(-1, 3))
    w = Walk.begin(list(C0), [3.75, 1.25, 0.25], LEAF)
    assert w.steps() == STEPS_OF_THE_CAPPED_RAY
    return out


def mixed_rays(n=None):
    """every case side by side in one array, so that the lanes of a wavefront differ; tiled or cut to n rays"""
    cases = ray_cases()
    order = [k for k in sorted(cases) if k not in ("one_run", "alternating_abab", "short_even_lanes")]
    o = np.concatenate([cases[k][0] for k in order] + [cases["short_even_lanes"][0][:10], cases["one_run"][0][:7]])
    e = np.concatenate([cases[k][1] for k in order] + [cases["short_even_lanes"][1][:10], cases["one_run"][1][:7]])
    if n is not None:
        reps = -(-n // len(o)) if n else 1
        o, e = np.tile(o, (reps, 1))[:n], np.tile(e, (reps, 1))[:n]
    return o, e


PARAM_VARIANTS = {
    "default": {},
    "skip_start_1": dict(skip_start=1),
    "skip_start_3": dict(skip_start=3),
    "unknown_stops": dict(unknown_stops=1),
    "max_steps_0": dict(max_steps=0),
    "max_steps_exact": dict(max_steps=STEPS_OF_THE_CAPPED_RAY),
    "max_steps_one_less": dict(max_steps=STEPS_OF_THE_CAPPED_RAY - 1),
}
RAY_COUNTS = (0, 1, 63, 64, 65, 257)


def random_segments(seed=11, n=3000, reach=12.0):
    """(vox, origins, ends): a random map of voxels with random counts inside +-reach metres and segments between random points of
    the same box, some of them on lattice planes"""
    rng = np.random.default_rng(seed)
    side = int(reach / LEAF)
    vox = {}
    for v in rng.integers(-side, side, size=(1500, 3)).tolist():
        vox[pack([c + BIAS for c in v])] = [int(rng.integers(0, 3)), int(rng.integers(0, 4))]
    o, e = rng.uniform(-reach, reach, (n, 3)), rng.uniform(-reach, reach, (n, 3))
    on_lattice = rng.random((n, 3)) < 0.1
    o = np.where(on_lattice, np.round(o / LEAF) * LEAF, o)
    e = np.where(rng.random((n, 3)) < 0.1, np.round(e / LEAF) * LEAF, e)
    return vox, o, e


def room_model(leaf=0.25):
    """a closed room around the origin, seen from inside: (model, cloud, pose). The cloud is the centre of every voxel of a shell one
    voxel thick, so no walk, which crosses one face per step, leaves the room without standing in an OCCUPIED voxel"""
    half = np.array([12, 10, 6])
    g = np.stack(np.meshgrid(*[np.arange(-h - 1, h + 1) for h in half], indexing="ij"), axis=-1).reshape(-1, 3)
    shell = g[((g < -half) | (g >= half)).any(axis=1)]
    pose = np.array([0.0, 0.0, 0.0, 1.0, 0.1, -0.05, 0.02])
    cloud = (shell + 0.5) * leaf - pose[4:]
    m = OM.OccupancyModel(leaf=leaf, min_range=0.1, max_range=30.0, end_margin=0.0)
    m.add(cloud, poses=pose[None])
    assert m.stats()["rays_hit"] == len(shell) == sum(1 for v in m.vox.values() if v[0])
    return m, cloud, pose


# ---- tests/hostcheck_raycast: raycast_math.h compiled by g++ -------------------------------------------------------------------------
HOSTCHECK_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck_raycast")
_lib = None


def hostcheck_lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", HOSTCHECK_DIR])
        _lib = C.CDLL(os.path.join(HOSTCHECK_DIR, "libhostcheck_raycast.so"))
    return _lib
