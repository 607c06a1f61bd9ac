"""Shared by the map upkeep tests: the room surface generator of tests/test_gpu_index_insert.py, and the numpy model of the
voxel filter that the kernels are compared with by equality (include/loamx.h, "map upkeep")."""
import numpy as np

BIAS = 1 << 20
BOX_LO, BOX_HI = np.array([-10.0, -8.0, -2.0]), np.array([10.0, 8.0, 4.0])
IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


def surface_points(rng, n):
    """walls and floor of a room, jittered: voxels of very different populations"""
    u = rng.uniform(0, 1, (n, 3)) * (BOX_HI - BOX_LO) + BOX_LO
    face = rng.integers(0, 3, n)
    u[np.arange(n), face] = np.where(rng.random(n) < 0.5, BOX_LO[face], BOX_HI[face]) + rng.normal(size=n) * 0.01
    return np.clip(u, BOX_LO - 0.05, BOX_HI + 0.05)


def voxel_keys(p, leaf):
    """(keys, ok): keys = pack(np.floor(p / leaf)); ok = every |v| < 2^20 (false for NaN / Inf)"""
    with np.errstate(all="ignore"):
        v = np.floor(np.asarray(p, dtype=np.float64).reshape(-1, 3) / leaf)
        ok = np.all(np.abs(v) < BIAS, axis=1)
    b = np.where(ok[:, None], v, 0.0).astype(np.int64) + BIAS
    return ((b[:, 0] << 42) | (b[:, 1] << 21) | b[:, 2]).astype(np.uint64), ok


def kept_indices(p, leaf, occupied=None):
    """input indices the filter keeps, ascending: the first point of every voxel, minus the voxels in `occupied` (a sorted
    array of keys or None); leaf <= 0 keeps everything"""
    n = len(p)
    if leaf <= 0:
        return np.arange(n)
    keys, ok = voxel_keys(p, leaf)
    cand = np.flatnonzero(ok)
    uniq, first = np.unique(keys[cand], return_index=True)
    if occupied is not None and len(occupied):
        first = first[~np.isin(uniq, occupied)]
    return np.sort(cand[first])


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def small_pose(rng, angle=0.02, shift=0.3):
    """a unit quaternion a few hundredths of a radian from the identity + a translation"""
    q = np.concatenate([rng.normal(size=3) * angle, [1.0]])
    return np.concatenate([q / np.linalg.norm(q), rng.normal(size=3) * shift])


class MapModel:
    """One feature kind of a map: its point array and, per leaf asked for, the occupied voxel keys of ALL its points."""

    def __init__(self, pts):
        self.pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3).copy()

    def occupied(self, leaf):
        keys, ok = voxel_keys(self.pts, leaf)
        assert ok.all()
        return np.unique(keys)

    def insert(self, pts):
        self.pts = np.concatenate([self.pts, np.asarray(pts).reshape(-1, 3)])

    def insert_filtered(self, moved, leaf):
        """moved: the transformed points (the library's own leaf <= 0 output); returns the number added"""
        keep = kept_indices(moved, leaf, self.occupied(leaf) if leaf > 0 else None)
        self.insert(moved[keep])
        return len(keep)

    def crop(self, lo, hi):
        m = np.all((self.pts >= lo) & (self.pts <= hi), axis=1)
        removed = int((~m).sum())
        self.pts = np.ascontiguousarray(self.pts[m])
        return removed
