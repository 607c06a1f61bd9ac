"""The rule of the surfel map (include/loamx.h, "surfel map") in Python. Steps 1 to 3 are the cloud map's (cloudmap_common:
validity, pose_act, cells, pack); the sums are Python ints (numpy uint64 / int64 where a whole call is folded at once: no sum can
wrap, see the header); surfel_finish is plain Python floats, one operation per statement in the header's order, math.sqrt the only
library call, the 128-bit numerator a Python int that goes to float as float(hi) * 2.0**64 + float(lo). Everything is compared by
equality. The map is a dict keyed by voxel: insertion order IS the rule's voxel order. No code shared with the kernels.
Also: the shared cases, and the binding of tests/hostcheck_surfel (surfel_math.h compiled by g++ as a program of its own)."""
import math
import os
import subprocess
import tempfile

import numpy as np

import cloudmap_common as CM

UNIT = 65536.0
VIEW_UNIT = 256.0
VIEW_CLAMP = 1073741824.0
TWO64 = 18446744073709551616.0
DEFAULTS = (0.5, 0.5, 120.0)
STAT_NAMES = CM.STAT_NAMES
CHUNK_CLOUDS = 256        # clouds per launch of an add
CHUNK_POINTS = 1 << 22    # points per launch of an add
SURFEL_DTYPE = np.dtype([("mean", np.float64, 3), ("cov", np.float64, 6), ("eval", np.float64, 3), ("normal", np.float64, 3),
                         ("count", np.uint32), ("first", np.uint32)])
assert SURFEL_DTYPE.itemsize == 128


# ---- per point ----------------------------------------------------------------------------------------------------------------
def view_terms(o, moved, leaf):
    """w (n, 3) int64: floor(clamp(((o - p') / leaf) 256)), the clamp as the header writes it"""
    with np.errstate(all="ignore"):
        d = np.asarray(o, dtype=np.float64)[None, :] - moved
        t = d / leaf
        x = t * VIEW_UNIT
        x = np.where(x >= -VIEW_CLAMP, x, -VIEW_CLAMP)
        x = np.where(x > VIEW_CLAMP, VIEW_CLAMP, x)
    return np.floor(x).astype(np.int64)


def point_terms(p, pose, leaf, min_range, max_range):
    """(what (n,), v (n, 3) int64, key (n,) uint64, q (n, 3) uint64, w (n, 3) int64) of one cloud; q and w are 0 where what != USED"""
    what = CM.validity(p, min_range, max_range)
    moved = p if pose is None else CM.pose_act(pose, p)
    ok, v, u = CM.cells(moved, leaf)
    what = np.where((what == CM.USED) & ~ok, CM.OUTSIDE, what)
    used = what == CM.USED
    q = np.where(used[:, None], u >> np.uint64(16), np.uint64(0)).astype(np.uint64)
    o = np.zeros(3) if pose is None else np.asarray(pose, dtype=np.float64)[4:7]
    w = np.where(used[:, None], view_terms(o, np.where(used[:, None], moved, 0.0), leaf), 0).astype(np.int64)
    return what, v, CM.pack(v), q, w


PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # xx xy xz yy yz zz


# ---- surfel_finish ------------------------------------------------------------------------------------------------------------
def numerator(count, S, sa, sb):
    """(N as a Python int, N as the header converts it to float)"""
    N = count * S - sa * sb
    mag = -N if N < 0 else N
    hi, lo = mag >> 64, mag & 0xFFFFFFFFFFFFFFFF
    assert hi < (1 << 64)
    a = float(hi) * TWO64
    d = a + float(lo)
    return N, (-d if N < 0 else d)


def _rotate(app, aqq, apq, arp, arq, vp, vq):
    """jacobi_rotate of reg_math.h; vp, vq: lists of three (columns p and q of V), changed in place"""
    if apq == 0.0:
        return app, aqq, apq, arp, arq
    num = aqq - app
    den = 2.0 * apq
    theta = num / den
    sign = 1.0 if theta >= 0.0 else -1.0
    tt = theta * theta
    tt1 = tt + 1.0
    root = math.sqrt(tt1)
    den2 = abs(theta) + root
    t = sign / den2
    t2 = t * t
    t21 = t2 + 1.0
    c = 1.0 / math.sqrt(t21)
    s = t * c
    tapq = t * apq
    app_n = app - tapq
    aqq_n = aqq + tapq
    x1 = c * arp
    x2 = s * arq
    arp_n = x1 - x2
    y1 = s * arp
    y2 = c * arq
    arq_n = y1 + y2
    for k in range(3):
        a, b = vp[k], vq[k]
        ca = c * a
        sb = s * b
        vp[k] = ca - sb
        sa = s * a
        cb = c * b
        vq[k] = sa + cb
    return app_n, aqq_n, 0.0, arp_n, arq_n


def eigen(cov):
    """(eval ascending, the column of the smallest, sweeps) of the symmetric matrix cov = (xx xy xz yy yz zz)"""
    a00, a01, a02, a11, a12, a22 = cov
    c0, c1, c2 = [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]  # columns of V
    sweeps = 0
    for _ in range(32):
        if a01 == 0.0 and a02 == 0.0 and a12 == 0.0:
            break
        sweeps += 1
        a00, a11, a01, a02, a12 = _rotate(a00, a11, a01, a02, a12, c0, c1)
        a00, a22, a02, a01, a12 = _rotate(a00, a22, a02, a01, a12, c0, c2)
        a11, a22, a12, a01, a02 = _rotate(a11, a22, a12, a01, a02, c1, c2)
    e = [(a00, c0), (a11, c1), (a22, c2)]
    if e[1][0] < e[0][0]:
        e[0], e[1] = e[1], e[0]
    if e[2][0] < e[1][0]:
        e[1], e[2] = e[2], e[1]
        if e[1][0] < e[0][0]:
            e[0], e[1] = e[1], e[0]
    return [e[0][0], e[1][0], e[2][0]], list(e[0][1]), sweeps


def finish(v, s, S, W, count, first, leaf):
    """one SURFEL_DTYPE record as a tuple; v, s, S, W: Python ints"""
    dn = float(count)
    h = leaf / UNIT
    mean = []
    for a in range(3):
        r = float(s[a]) / dn
        r = r / UNIT
        r = float(v[a]) + r
        mean.append(r * leaf)
    dn2 = dn * dn
    h2 = h * h
    cov = []
    for k, (a, b) in enumerate(PAIRS):
        _, nf = numerator(count, S[k], s[a], s[b])
        c = nf / dn2
        cov.append(c * h2)
    ev, n, _ = eigen(cov)
    d0 = n[0] * float(W[0])
    d1 = n[1] * float(W[1])
    d2 = n[2] * float(W[2])
    dot = d0 + d1
    dot = dot + d2
    flip = dot < 0.0
    if dot == 0.0:
        big = n[0]
        if abs(n[1]) > abs(big):
            big = n[1]
        if abs(n[2]) > abs(big):
            big = n[2]
        flip = big < 0.0
    if flip:
        n = [-n[0], -n[1], -n[2]]
    return (mean, cov, ev, n, count, first)


def distance(rec, p):
    """normal . (p - mean), left to right; rec: a finish tuple"""
    mean, n = rec[0], rec[3]
    d0 = n[0] * (float(p[0]) - mean[0])
    d1 = n[1] * (float(p[1]) - mean[1])
    d2 = n[2] * (float(p[2]) - mean[2])
    d = d0 + d1
    return d + d2


def records(tuples):
    out = np.zeros(len(tuples), dtype=SURFEL_DTYPE)
    for i, t in enumerate(tuples):
        out[i] = (t[0], t[1], t[2], t[3], t[4], t[5])
    return out


# ---- the map ------------------------------------------------------------------------------------------------------------------
class SurfelMapModel:
    def __init__(self, leaf=DEFAULTS[0], min_range=DEFAULTS[1], max_range=DEFAULTS[2]):
        self.leaf, self.min_range, self.max_range = float(leaf), float(min_range), float(max_range)
        self.clear()

    def clear(self):
        self.vox = {}  # key -> [v (3 ints), s (3 ints), S (6 ints), W (3 ints), count, first], in order of first appearance
        self.offered = self.used = self.invalid = self.range = self.outside = 0
        self.plain_claims = self.wave_claims = 0

    def add(self, points, offsets=None, poses=None):
        """points: (n, k >= 3) float64 or float32; offsets: n_clouds + 1 point offsets (None: one cloud); poses: (n_clouds, 7) or None.
        The claims of both forms are counted as the kernel's launches cut the call: CHUNK_CLOUDS clouds at a time, their points
        CHUNK_POINTS at a time, the wavefronts of a launch counted from its first point."""
        pts = np.asarray(points)[:, :3].astype(np.float64)
        offsets = [0, len(pts)] if offsets is None else [int(o) for o in offsets]
        nc = len(offsets) - 1
        whats, keys, vs, qs, ws = [], [], [], [], []
        for c in range(nc):
            p = pts[offsets[c]:offsets[c + 1]]
            what, v, key, q, w = point_terms(p, None if poses is None else poses[c], self.leaf, self.min_range, self.max_range)
            whats.append(what), keys.append(key), vs.append(v), qs.append(q), ws.append(w)
        if not whats:
            return
        what, key, v = np.concatenate(whats), np.concatenate(keys), np.concatenate(vs)
        q, w = np.concatenate(qs), np.concatenate(ws)
        used = what == CM.USED
        self.invalid += int((what == CM.INVALID).sum())
        self.range += int((what == CM.RANGE).sum())
        self.outside += int((what == CM.OUTSIDE).sum())
        self.used += int(used.sum())
        # the claims, launch by launch
        self.plain_claims += int(used.sum())
        for c0 in range(0, nc, CHUNK_CLOUDS):
            lo, hi = offsets[c0] - offsets[0], offsets[min(c0 + CHUNK_CLOUDS, nc)] - offsets[0]
            for a in range(lo, hi, CHUNK_POINTS):
                b = min(a + CHUNK_POINTS, hi)
                self.wave_claims += CM.wave_runs(used[a:b], key[a:b])
        # the sums, folded per voxel of the call (exact in 64 bits), then into the dict in order of first appearance
        idx = np.flatnonzero(used)
        if len(idx):
            uk, first_pos, inv = np.unique(key[idx], return_index=True, return_inverse=True)
            order = np.argsort(inv, kind="stable")
            starts = np.concatenate([[0], np.flatnonzero(np.diff(inv[order])) + 1])
            qq = q[idx][order]
            ww = w[idx][order]
            s = np.add.reduceat(qq, starts, axis=0)
            S = np.stack([np.add.reduceat(qq[:, a] * qq[:, b], starts) for a, b in PAIRS], axis=1)
            W = np.add.reduceat(ww, starts, axis=0)
            counts = np.diff(np.concatenate([starts, [len(order)]]))
            for j in np.argsort(first_pos, kind="stable"):
                g = self.offered + int(idx[first_pos[j]])
                e = self.vox.get(int(uk[j]))
                if e is None:
                    e = self.vox[int(uk[j])] = [v[idx[first_pos[j]]].tolist(), [0] * 3, [0] * 6, [0] * 3, 0, g]
                for a in range(3):
                    e[1][a] += int(s[j, a])
                    e[3][a] += int(W[j, a])
                for a in range(6):
                    e[2][a] += int(S[j, a])
                e[4] += int(counts[j])
        self.offered += offsets[-1] - offsets[0]

    def entries(self, min_points=1):
        return [e for e in self.vox.values() if e[4] >= min_points]

    def emit(self, min_points=1, capacity=None):
        """(records, n) as SurfelMap.emit"""
        es = self.entries(min_points)
        n = len(es)
        es = es if capacity is None else es[:capacity]
        return records([finish(e[0], e[1], e[2], e[3], e[4], e[5], self.leaf) for e in es]), n

    def query(self, points, min_points=1):
        """(records, distance, count) of the voxels of (n, k >= 3) float64 points"""
        p = np.asarray(points, dtype=np.float64)[:, :3]
        ok, v, _ = CM.cells(p, self.leaf)
        key = CM.pack(v)
        out, dist, cnt = np.zeros(len(p), dtype=SURFEL_DTYPE), np.zeros(len(p)), np.zeros(len(p), dtype=np.uint32)
        for i in range(len(p)):
            e = self.vox.get(int(key[i])) if ok[i] else None
            if e is None or e[4] < min_points:
                continue
            r = finish(e[0], e[1], e[2], e[3], e[4], e[5], self.leaf)
            out[i] = (r[0], r[1], r[2], r[3], r[4], r[5])
            dist[i], cnt[i] = distance(r, p[i]), e[4]
        return out, dist, cnt

    def stats(self):
        return dict(voxels=len(self.vox), points_offered=self.offered, points_used=self.used, invalid=self.invalid, range=self.range,
                    outside=self.outside, overflow=0)


same_bytes = CM.same_bytes
assert_stats_equal = CM.assert_stats_equal


def assert_records_equal(got, want, what=""):
    """two SURFEL_DTYPE arrays byte for byte, saying which field of which voxel differs first"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == SURFEL_DTYPE, (what, got.shape, want.shape)
    if same_bytes(got, want):
        return
    for name in SURFEL_DTYPE.names:
        g, w = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        bits = np.uint64 if g.dtype == np.float64 else np.uint32
        bad = np.flatnonzero((g.view(bits) != w.view(bits)).reshape(len(got), -1).any(axis=1))
        assert not len(bad), (what, name, "voxel", int(bad[0]), g[bad[0]].tolist(), w[bad[0]].tolist(), f"{len(bad)} of {len(got)} differ")
    raise AssertionError((what, "records differ outside their fields"))


def assert_emit_equal(got, want, what=""):
    assert got[1] == want[1], (what, got[1], want[1])
    assert_records_equal(got[0], want[0], what)


# ---- the shared cases: {name: (leaf, points (n, 3), pose7 or None)} -----------------------------------------------------------------
def _lattice(leaf, corner, steps):
    """points at corner + steps / 65536 voxel edges: offsets that are exact in the 16-bit grid (steps: (n, 3) ints in 0 .. 65535);
    half a step is added so that the floor lands on the step whatever the division's last bit does"""
    return (np.asarray(corner, dtype=np.float64) + (np.asarray(steps, dtype=np.float64) + 0.5) / UNIT) * leaf


def shared_cases():
    rng = np.random.default_rng(4181)
    unit = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
    cases = {}
    one = np.array([[1.3, 2.6, 0.7]])
    cases["one_point"] = (1.0, one, None)
    cases["two_points"] = (1.0, np.array([[1.3, 2.6, 0.7], [1.8, 2.1, 0.2]]), unit)
    cases["three_points"] = (1.0, np.array([[1.3, 2.6, 0.7], [1.8, 2.1, 0.2], [1.1, 2.9, 0.4]]), unit)
    line = np.arange(8)[:, None] * 1000 + 500
    cases["collinear_x"] = (0.5, _lattice(0.5, (3, -2, 1), line * [1, 0, 0] + [0, 77, 99]), unit)
    cases["collinear_diagonal"] = (0.5, _lattice(0.5, (3, -2, 1), line * [1, 1, 1]), unit)
    gx, gy = np.meshgrid(np.arange(6) * 4096 + 100, np.arange(6) * 4096 + 100)
    flat = np.stack([gx.ravel(), gy.ravel(), np.full(36, 31000)], axis=1)
    cases["coplanar_xy"] = (2.0, _lattice(2.0, (-4, 0, 0), flat), unit)              # eigenvalues (0, s, s): the tie order
    cases["coplanar_yz"] = (2.0, _lattice(2.0, (-4, 0, 0), flat[:, [2, 0, 1]]), unit)
    cases["coplanar_zx"] = (2.0, _lattice(2.0, (-4, 0, 0), flat[:, [1, 2, 0]]), unit)
    cube = np.array([[x, y, z] for x in (1000, 9000) for y in (1000, 9000) for z in (1000, 9000)])
    cases["cube_equal_eigenvalues"] = (1.0, _lattice(1.0, (0, 0, 0), cube), unit)
    # a diagonal covariance in each of the six orders of its three spreads
    spreads = (300, 2000, 12000)
    for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        sx, sy, sz = (spreads[k] for k in perm)
        box = np.array([[32000 + a * sx, 32000 + b * sy, 32000 + c * sz] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)])
        cases["diagonal_%d%d%d" % perm] = (0.25, _lattice(0.25, (7, 7, -7), box), unit)
    # q at 0 and 65535 on each axis
    for a in range(3):
        st = np.full((4, 3), 30000)
        st[:, a] = (0, 0, 65535, 65535)
        st[:, (a + 1) % 3] = (10, 50000, 10, 50000)
        cases["q_edges_axis_%d" % a] = (1.0, _lattice(1.0, (-1, -1, -1), st), unit)
    # t = -1e-20 (v = -1, frac exactly 1.0, the clamped offset) and negative voxels
    cases["minus_1e_20"] = (1.0, np.array([[-1e-20, 3.5, 0.5], [-0.25, 3.5, 0.5], [-1e-20, -1e-20, -1e-20], [-0.5, -0.5, -0.5]]), unit)
    # |n0| == |n1| exactly (a plane x - y = const: the first rotation has theta = 0): the lowest axis decides a dot of 0
    tie = np.array([[20000 + a, 30000 + a, z] for a in (0, 4000, 8000, 12000) for z in (1000, 50000)])
    cases["plane_x_minus_y"] = (1.0, _lattice(1.0, (1, 1, 1), tie), unit)
    cases["negative_voxels"] = (0.3, rng.uniform(-9.0, -8.0, (200, 3)), unit)
    # the sign path of the numerator: x up while y down
    anti = np.stack([np.arange(10) * 5000 + 100, 60000 - np.arange(10) * 5000, np.arange(10) * 100 + 7], axis=1)
    cases["negative_covariance"] = (1.0, _lattice(1.0, (2, 2, 2), anti), unit)
    # the view: seen from below / above / sideways, dot == 0 (no poses: W = -p' steps; a plane through the origin's voxel row)
    floor_pts = _lattice(1.0, (0, 0, 3), flat)
    cases["seen_from_below"] = (1.0, floor_pts - [0.0, 0.0, -50.0], np.array([0.0, 0, 0, 1.0, 0, 0, -50.0]))  # (given in the sensor's frame)
    cases["seen_from_above"] = (1.0, floor_pts - [0.0, 0.0, 50.0], np.array([0.0, 0, 0, 1.0, 0, 0, 50.0]))
    cases["no_poses"] = (1.0, floor_pts, None)
    # dot == 0 exactly: the sensor in the plane (o - p' has no z part: W2 = 0, the normal is +-z). floor(x) of -0.0 is 0.
    in_plane = np.stack([flat[:, 0], flat[:, 1], np.zeros(36)], axis=1) / UNIT
    cases["dot_zero_sensor_in_plane"] = (1.0, in_plane + [0.0, 0.0, 0.0], None)
    # non-unit quaternions (used as given) and a far-away pose that reaches the view clamp
    cases["non_unit_quaternion"] = (0.5, rng.uniform(-2, 2, (300, 3)), np.array([0.1, -0.2, 0.3, 1.1, 0.5, -0.5, 0.25]))
    cases["double_quaternion"] = (0.5, rng.uniform(-2, 2, (300, 3)), np.array([0.0, 0.0, 0.0, 2.0, 1.0, 1.0, 1.0]))
    # random clouds
    cases["random_dense"] = (0.5, rng.normal(size=(3000, 3)) * [3.0, 3.0, 0.4], np.array([0.02, -0.01, 0.2, 0.97, 1.0, -2.0, 0.5]))
    return cases


def big_voxel(n=140000):
    """n points of ONE voxel, half at the lowest and half at the highest offset: count S and N reach 2^64. (leaf, points)"""
    lo, hi = np.full((n // 2, 3), 0.5 / UNIT), np.full((n - n // 2, 3), (65535 + 0.5) / UNIT)
    pts = np.concatenate([lo, hi]) + [4.0, 4.0, 4.0]
    return 1.0, pts[np.random.default_rng(7).permutation(n)]


# ---- tests/hostcheck_surfel: surfel_math.h compiled by g++ ---------------------------------------------------------------------------
HOSTCHECK_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck_surfel")
POINT_IN = np.dtype([("n", np.uint64), ("leaf", np.float64), ("min_r2", np.float64), ("max_r2", np.float64), ("has_pose", np.uint64),
                     ("pose", np.float64, 7)])
POINT_OUT = np.dtype([("what", np.uint64), ("key", np.uint64), ("m", np.uint64, 12)])
FINISH_IN = np.dtype([("key", np.uint64), ("s", np.uint64, 3), ("S", np.uint64, 6), ("W", np.int64, 3), ("count", np.uint32), ("first", np.uint32),
                      ("leaf", np.float64)])


def hostcheck_program(san=False):
    subprocess.check_call(["make", "-s", "-C", HOSTCHECK_DIR] + (["san"] if san else []))
    return os.path.join(HOSTCHECK_DIR, "hostcheck_surfel_san" if san else "hostcheck_surfel")


def _run(program, mode, blob, out_dtype, n):
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(blob)
        r = subprocess.run([program, mode, fin, fout], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        out = np.fromfile(fout, dtype=out_dtype)
    assert len(out) == n
    return out


def hostcheck_points(program, pts, pose, leaf, min_range, max_range):
    """POINT_OUT per point: cloud_validity, pose_act, cloud_cell and surfel_point of surfel_math.h"""
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    head = np.zeros(1, dtype=POINT_IN)
    head["n"], head["leaf"], head["min_r2"], head["max_r2"] = len(pts), leaf, min_range * min_range, max_range * max_range
    if pose is not None:
        head["has_pose"], head["pose"] = 1, pose
    return _run(program, "points", head.tobytes() + pts.tobytes(), POINT_OUT, len(pts))


def hostcheck_finish(program, entries, leaf):
    """surfel_finish of surfel_math.h on the model's entries [v, s, S, W, count, first]"""
    rec = np.zeros(len(entries), dtype=FINISH_IN)
    for i, e in enumerate(entries):
        rec[i] = (int(CM.pack(np.array([e[0]], dtype=np.int64))[0]), e[1], e[2], e[3], e[4], e[5], leaf)
    return _run(program, "finish", rec.tobytes(), SURFEL_DTYPE, len(entries))
