"""The rule of the cloud organiser (include/loamx.h, "unordered clouds into scans") in plain numpy: an n x W sign matrix for the
columns, an n x (H + 1) comparison matrix for the lines, a sort for the winners. It reads the two tables the library hands out
(loamx_scan_layout_tables), so it depends on nobody's cos or tan, and it ASSERTS what the rule takes for granted: exactly one
column per valid point (W > 1) and answers that are monotone along the line boundaries. No code shared with the kernels."""
import numpy as np

INVALID, OUTSIDE = 0xFFFFFFFE, 0xFFFFFFFF
NO_POINT = 0xFFFFFFFF
KEEP_FIRST, KEEP_NEAREST = 0, 1


def classify(points, col_dirs, line_tans, clockwise=False, rings=None, ring_map=None, chunk=None):
    """points (n, >= 3), any float dtype (widened first) -> (cell (n,) uint32: line * W + column, INVALID or OUTSIDE; r2 (n,))"""
    p = np.asarray(points)[:, :3].astype(np.float64)
    col_dirs, line_tans = np.asarray(col_dirs, dtype=np.float64).reshape(-1, 2), np.asarray(line_tans, dtype=np.float64)
    W, H = len(col_dirs), len(line_tans) - 1
    n = len(p)
    chunk = chunk or max(64, (1 << 21) // W)  # (the sign matrix of a chunk stays at 16 MB)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        rho2 = x * x + y * y
        r2 = rho2 + z * z
        valid = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & np.isfinite(r2) & (rho2 >= 1e-100)
    cell = np.full(n, INVALID, dtype=np.uint32)
    sgn = -1.0 if clockwise else 1.0
    ux, uy = col_dirs[:, 0], col_dirs[:, 1]
    for a in range(0, n, chunk):
        v = np.flatnonzero(valid[a:a + chunk]) + a
        if not len(v):
            continue
        xv, yv, zv = x[v], y[v], z[v]
        if W == 1:
            col = np.zeros(len(v), dtype=np.int64)
        else:
            with np.errstate(over="ignore"):
                s = sgn * (ux[None, :] * yv[:, None] - uy[None, :] * xv[:, None]) >= 0
            hit = s & ~np.roll(s, -1, axis=1)
            assert (hit.sum(axis=1) == 1).all(), "a valid point without exactly one column"
            col = hit.argmax(axis=1)
        if rings is None:
            with np.errstate(over="ignore"):
                ge = zv[:, None] >= line_tans[None, :] * np.sqrt(rho2[v])[:, None]
            assert not (ge[:, 1:] & ~ge[:, :-1]).any(), "the line comparisons are not monotone"
            cnt = ge.sum(axis=1)
            line = cnt - 1
            out = (cnt == 0) | (cnt == H + 1)
        else:
            ring = np.asarray(rings)[v].astype(np.int64)
            if ring_map is None:
                line, out = ring, ring >= H
            else:
                rm = np.asarray(ring_map).astype(np.int64)
                beyond = ring >= len(rm)
                line = np.where(beyond, 0, rm[np.minimum(ring, max(len(rm) - 1, 0))] if len(rm) else 0)
                out = beyond | (line == 0xFFFF) | (line >= H)
        cell[v] = np.where(out, OUTSIDE, np.where(out, 0, line) * W + col).astype(np.uint32)
    return cell, r2


def organize(points, H, W, col_dirs, line_tans, clockwise=False, rings=None, ring_map=None, keep=KEEP_FIRST):
    """one cloud -> (scan (H W, 3) in the cloud's dtype, src_idx (H W,) uint32, stats uint32 [filled, invalid, outside, collisions])"""
    pts = np.asarray(points)
    n = len(pts)
    scan, src = np.zeros((H * W, 3), dtype=pts.dtype), np.full(H * W, NO_POINT, dtype=np.uint32)
    if n == 0:
        return scan, src, np.zeros(4, dtype=np.uint32)
    cell, r2 = classify(pts, col_dirs, line_tans, clockwise, rings, ring_map)
    placed = np.flatnonzero(cell < INVALID)
    if keep == KEEP_NEAREST:
        order = placed[np.lexsort((placed, r2[placed], cell[placed]))]
    else:
        order = placed[np.lexsort((placed, cell[placed]))]
    first = np.ones(len(order), dtype=bool)
    first[1:] = cell[order[1:]] != cell[order[:-1]]
    win = order[first]
    scan[cell[win]] = pts[win, :3]
    src[cell[win]] = win
    invalid, outside = int((cell == INVALID).sum()), int((cell == OUTSIDE).sum())
    return scan, src, np.array([len(win), invalid, outside, n - len(win) - invalid - outside], dtype=np.uint32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def fan_elevations(H, fan_deg):
    """the beam elevations of tests/outdoor_scenes.beam_directions for a fan (top, bottom) in degrees"""
    top, bottom = fan_deg
    return np.radians(bottom + (top - bottom) * np.arange(H) / (H - 1))


def random_cloud(rng, n, lo=-30.0, hi=30.0, zscale=0.25):
    p = rng.uniform(lo, hi, (n, 3))
    p[:, 2] *= zscale
    return p
