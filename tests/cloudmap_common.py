"""The rule of the cloud map (include/loamx.h, "cloud map") in plain numpy: validity, transform, voxel, 32-bit offset, integer
sums and the centroid, float64 operations one at a time in the header's order (numpy's elementwise loops round every
operation on its own), so everything is compared by equality. The map itself is a dict keyed by voxel: Python dicts keep
insertion order, which IS the rule's voxel order. No code shared with the kernels. Also: the binding of
tests/hostcheck_cloudmap."""
import ctypes as C
import os
import subprocess

import numpy as np

BIAS = 1 << 20
UNIT = 4294967296.0
U32_MAX = 0xFFFFFFFF
USED, INVALID, RANGE, OUTSIDE = range(4)
DEFAULTS = (0.2, 0.5, 120.0)
STAT_NAMES = ("voxels", "points_offered", "points_used", "invalid", "range", "outside", "overflow")


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def pose_act(pose, p):
    """Pose3d::act on (n, 3) points: v + w (2 u x v) + u x (2 u x v) + t, the quaternion as given"""
    pose = np.asarray(pose, dtype=np.float64)
    v = tuple(p[:, k] for k in range(3))
    u = (pose[0], pose[1], pose[2])
    with np.errstate(all="ignore"):  # (dropped points are transformed too, and thrown away)
        uv = _cross(u, v)
        uv = tuple(c + c for c in uv)
        cc = _cross(u, uv)
        return np.stack([((v[k] + pose[3] * uv[k]) + cc[k]) + pose[4 + k] for k in range(3)], axis=1)


def validity(p, min_range, max_range):
    """per point USED / INVALID / RANGE (step 1); p: (n, 3) float64"""
    with np.errstate(all="ignore"):
        r2 = p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2]
        finite = np.isfinite(p).all(axis=1) & np.isfinite(r2)
        in_range = (r2 >= min_range * min_range) & (r2 <= max_range * max_range)
    return np.where(~finite, INVALID, np.where(~in_range, RANGE, USED))


def cells(p, leaf):
    """(ok, v (n, 3) int64, u (n, 3) uint64): steps 3 and 4; v and u are 0 where not ok"""
    with np.errstate(all="ignore"):
        t = p / leaf
        v = np.floor(t)
        ok = np.all(np.abs(v) < BIAS, axis=1)
        frac = np.where(ok[:, None], t - v, 0.0)
        u = np.minimum(np.floor(frac * UNIT), UNIT - 1.0)  # (floor(frac 2^32) <= 2^32 is exact in float64; the clamp too)
    return ok, np.where(ok[:, None], v, 0.0).astype(np.int64), u.astype(np.uint64)


def pack(v):
    b = (v + BIAS).astype(np.uint64)
    return (b[:, 0] << np.uint64(42)) | (b[:, 1] << np.uint64(21)) | b[:, 2]


def centroid(v, sums, count, leaf):
    """step 6; v (m, 3) int64, sums (m, 3) uint64, count (m,)"""
    return (v.astype(np.float64) + (sums.astype(np.float64) / np.asarray(count).astype(np.float64)[:, None]) / UNIT) * leaf


def wave_runs(ok, key):
    """the claims of the run-combining form for the points of ONE call (fewer than 2^22): a point with a voxel opens a run
    unless the point before it is in the same wavefront (64 consecutive points of the call), has a voxel and has the same key"""
    ok, key = np.asarray(ok, dtype=bool), np.asarray(key)
    head = ok.copy()
    same = ok[1:] & ok[:-1] & (key[1:] == key[:-1])
    same[63::64] = False  # (point 64 k is lane 0 of its wavefront)
    head[1:] &= ~same
    return int(head.sum())


class CloudMapModel:
    def __init__(self, leaf=DEFAULTS[0], min_range=DEFAULTS[1], max_range=DEFAULTS[2]):
        self.leaf, self.min_range, self.max_range = float(leaf), float(min_range), float(max_range)
        self.clear()

    def clear(self):
        self.vox = {}  # key -> [v (3 ints), sums (3 ints), count, first], in order of first appearance
        self.offered = self.used = self.invalid = self.range = self.outside = 0

    def add(self, points, offsets=None, poses=None):
        """points: (n, k >= 3) float64 or float32; offsets: n_clouds + 1 point offsets (None: one cloud); poses: (n_clouds, 7) or None"""
        pts = np.asarray(points)[:, :3].astype(np.float64)
        offsets = [0, len(pts)] if offsets is None else [int(o) for o in offsets]
        g = self.offered
        for c in range(len(offsets) - 1):
            p = pts[offsets[c]:offsets[c + 1]]
            what = validity(p, self.min_range, self.max_range)
            moved = p if poses is None else pose_act(poses[c], p)
            ok, v, u = cells(moved, self.leaf)
            what = np.where((what == USED) & ~ok, OUTSIDE, what)
            self.invalid += int((what == INVALID).sum())
            self.range += int((what == RANGE).sum())
            self.outside += int((what == OUTSIDE).sum())
            keys = pack(v)
            for i in np.flatnonzero(what == USED):
                e = self.vox.get(int(keys[i]))
                if e is None:
                    self.vox[int(keys[i])] = [v[i].tolist(), [int(x) for x in u[i]], 1, g + int(i)]
                else:
                    for a in range(3):
                        e[1][a] += int(u[i, a])
                    e[2] += 1
                self.used += 1
            g += len(p)
        self.offered += offsets[-1] - offsets[0]

    def emit(self, min_points=1, capacity=None):
        """(xyz, count, first, n) as CloudMap.emit"""
        es = [e for e in self.vox.values() if e[2] >= min_points]
        n = len(es)
        es = es if capacity is None else es[:capacity]
        if not es:
            return np.empty((0, 3)), np.empty(0, dtype=np.uint32), np.empty(0, dtype=np.uint32), n
        v = np.array([e[0] for e in es], dtype=np.int64)
        sums = np.array([e[1] for e in es], dtype=np.uint64)
        count = np.array([e[2] for e in es], dtype=np.uint32)
        first = np.array([e[3] for e in es], dtype=np.uint32)
        return centroid(v, sums, count, self.leaf), count, first, n

    def stats(self):
        return dict(voxels=len(self.vox), points_offered=self.offered, points_used=self.used, invalid=self.invalid, range=self.range,
                    outside=self.outside, overflow=0)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_emit_equal(got, want, what=""):
    """two (xyz, count, first, n) results, byte for byte"""
    assert got[3] == want[3], (what, got[3], want[3])
    assert same_bytes(got[2], want[2]), (what, "first / order")
    assert same_bytes(got[1], want[1]), (what, "count")
    assert same_bytes(got[0], want[0]), (what, "centroids")


def assert_stats_equal(got, want, what=""):
    g = {n: int(got[n]) for n in STAT_NAMES}
    assert g == {n: int(want[n]) for n in STAT_NAMES}, (what, g, want)


# ---- tests/hostcheck_cloudmap: cloudmap_math.h compiled by g++ -----------------------------------------------------------------
HOSTCHECK_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck_cloudmap")
_lib = None


def hostcheck_lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", HOSTCHECK_DIR])
        _lib = C.CDLL(os.path.join(HOSTCHECK_DIR, "libhostcheck_cloudmap.so"))
    return _lib
