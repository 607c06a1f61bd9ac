"""The rule of place recognition (include/loamx.h, "place recognition") in plain numpy: an n x S sign matrix for the sector, int64 /
uint64 sums, float64 operations one at a time. It reads the sector table the library hands out (loamx_place_db_sector_dirs), so
it depends on nobody's cos, and it ASSERTS what the rule takes for granted: exactly one sector per valid point. No code shared
with the kernels."""
import numpy as np

NO_ID = 0xFFFFFFFF
NO_KEY_DIST = 0xFFFFFFFFFFFFFFFF
COS_ONE = 1 << 30
MATCH_DTYPE = np.dtype([("id", np.uint32), ("shift", np.uint32), ("key_dist", np.uint64), ("distance", np.float64)])
DEFAULTS = dict(n_rings=20, n_sectors=60, max_range=80.0, z_offset=2.0, z_scale=64.0)


def classify(points, dirs, R, max_range, z_offset, z_scale):
    """points (n, >= 3), any float dtype (widened first) -> (cell (n,) int64: ring * S + sector, or -1 for a dropped point;
    code (n,) int64)"""
    p = np.asarray(points)[:, :3].astype(np.float64)
    dirs = np.asarray(dirs, dtype=np.float64).reshape(-1, 2)
    S, n = len(dirs), len(p)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    ring_scale = np.float64(R) / np.float64(max_range)
    cell, code = np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.int64)
    with np.errstate(all="ignore"):
        rho2 = x * x + y * y
        r2 = rho2 + z * z
        valid = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & np.isfinite(r2) & (rho2 >= 1e-100)
        f = np.sqrt(rho2) * ring_scale
        keep = valid & (f < R)
    v = np.flatnonzero(keep)
    if not len(v):
        return cell, code
    ring = np.floor(f[v]).astype(np.int64)
    with np.errstate(over="ignore"):
        s = (dirs[None, :, 0] * y[v, None] - dirs[None, :, 1] * x[v, None]) >= 0
    hit = s & ~np.roll(s, -1, axis=1)
    assert (hit.sum(axis=1) == 1).all(), "a valid point without exactly one sector"
    sector = hit.argmax(axis=1)
    with np.errstate(over="ignore"):
        h = np.floor((z[v] + np.float64(z_offset)) * np.float64(z_scale))
    h = np.where(h >= 0.0, np.minimum(h, 65534.0), 0.0)  # (h is never a NaN: every operand is finite, z_scale > 0)
    cell[v], code[v] = ring * S + sector, h.astype(np.int64) + 1
    return cell, code


def descriptor(points, dirs, n_rings=20, max_range=80.0, z_offset=2.0, z_scale=64.0, **_):
    """one cloud -> (R, S) uint16"""
    S = len(np.asarray(dirs).reshape(-1, 2))
    d = np.zeros(n_rings * S, dtype=np.int64)
    if len(points):
        cell, code = classify(points, dirs, n_rings, max_range, z_offset, z_scale)
        ok = cell >= 0
        np.maximum.at(d, cell[ok], code[ok])
    return d.astype(np.uint16).reshape(n_rings, S)


def ring_keys(desc):
    """(..., R, S) uint16 -> (..., R) uint32"""
    return np.asarray(desc).astype(np.int64).sum(axis=-1).astype(np.uint32)


def column_norms(desc):
    """(..., R, S) uint16 -> (..., S) uint64"""
    d = np.asarray(desc).astype(np.uint64)
    return (d * d).sum(axis=-2, dtype=np.uint64)


def key_distance(kq, ke):
    d = np.asarray(kq).astype(np.int64) - np.asarray(ke).astype(np.int64)
    return (d * d).sum(axis=-1).astype(np.uint64)


def cos_q(dot, nq, ne):
    """the quantised cosines of column pairs with both norms non-zero (uint64 arrays)"""
    den = np.sqrt(nq.astype(np.float64) * ne.astype(np.float64))
    c = dot.astype(np.float64) / den
    t = c * np.float64(COS_ONE)
    return np.where(t < COS_ONE, np.floor(np.minimum(t, np.float64(COS_ONE))), np.float64(COS_ONE)).astype(np.uint64)


def shift_distances(q, e):
    """(R, S) x (R, S) -> dist (S,) float64 over the shifts"""
    q64, e64 = np.asarray(q).astype(np.uint64), np.asarray(e).astype(np.uint64)
    S = q64.shape[1]
    nq, ne = column_norms(q), column_norms(e)
    dots = q64.T @ e64  # [j][j'], exact: at most 64 x 65535^2 < 2^38
    j = np.arange(S)
    dist = np.empty(S)
    for s in range(S):
        jj = (j + s) % S
        on = (nq > 0) & (ne[jj] > 0)
        m = int(on.sum())
        if m == 0:
            dist[s] = 1.0
            continue
        score = int(cos_q(dots[j[on], jj[on]], nq[on], ne[jj][on]).sum(dtype=np.uint64))
        dist[s] = np.float64(1.0) - np.float64(score) / (np.float64(m) * np.float64(COS_ONE))
    return dist


def pair_distance(q, e):
    """-> (distance, shift): the smallest over the shifts, the lowest shift on a tie"""
    d = shift_distances(q, e)
    s = int(np.argmin(d))  # (argmin takes the first of equal minima)
    return d[s], s


def search(query, entries, K, id_end=None):
    """one query (R, S) against entries (N, R, S) -> K MATCH_DTYPE records ascending by (distance, id)"""
    entries = np.asarray(entries)
    N = len(entries) if id_end is None else min(len(entries), int(id_end))
    out = np.zeros(K, dtype=MATCH_DTYPE)
    out["id"], out["shift"], out["key_dist"], out["distance"] = NO_ID, 0, NO_KEY_DIST, 2.0
    if N == 0:
        return out
    kd = key_distance(ring_keys(query)[None, :], ring_keys(entries[:N]))
    pick = np.lexsort((np.arange(N), kd))[:K]
    recs = []
    for i in pick:
        d, s = pair_distance(query, entries[i])
        recs.append((d, int(i), s, int(kd[i])))
    recs.sort(key=lambda r: (r[0], r[1]))
    for k, (d, i, s, key) in enumerate(recs):
        out[k] = (i, s, key, d)
    return out


def same_records(got, want, where=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (where, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (where, got.tolist(), want.tolist())


def random_cloud(rng, n, lo=-90.0, hi=90.0, z_lo=-4.0, z_hi=12.0):
    p = rng.uniform(lo, hi, (n, 3))
    p[:, 2] = rng.uniform(z_lo, z_hi, n)
    return p


def random_descriptors(rng, n, R, S, fill=0.7, hi=2000):
    d = rng.integers(1, hi, (n, R, S)).astype(np.uint16)
    d[rng.random((n, R, S)) > fill] = 0
    return d
