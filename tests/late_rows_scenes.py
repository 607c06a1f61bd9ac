"""Scenes for the late list of the plane fit (associate_fit_late_kernel, one row of 16 lanes per late query), the
smallest that reach each form of the row search, with the arithmetic that says why. Every scene is an assoc_scenes.Scene of the
mixed launch (a small edge pair beside a planar target of more than 512 points, k <= 5) at the identity pose; under the option
FORCE_LATE_VERIFY every selection round 1 hands to the fit takes the late list, so `late` is the number of queries round 1
finishes — which the g++ build of the kernels' functions counts (hostcheck_lib.knn_routes: `unverified`), so that a scene cannot
go vacuous unseen — and each scene says what that number is by construction.

Two layouts:
  * the wall of assoc_scenes (2 000 points on a plane, h = 0.44, ~150 candidates in a 3x3x3 block), and with it queries 100 m
    away, which are neither queued nor selected (count 0 in front of the search): they fill n_src without entering the list;
  * clusters in a box 100 m wide (three outliers at +-50 m; as assoc_scenes.trip_budget): fewer than 4 096 points cap the table
    at 16 n cells, the cell edge is 4.4 m or more, and a cluster of a few centimetres lies in ONE cell whose 3x3x3 block holds
    nothing else: the block's population is the cluster's, every neighbour within the 2 m radius lies inside the block, and its
    faces are farther than the radius: round 1 finishes every query there whatever it finds."""
import numpy as np

import assoc_scenes as S

FAR = np.array([100.0, 100.0, 100.0])
A = np.array([3.0, -2.0, 1.0])  # where the clusters of the box layout sit
OUTLIERS = np.array([[50.0, 50, 50], [-50, -50, -50], [50, -50, 0]])
ROW_CAP = 256  # reg_math.h kRow16Cap


def rows_per_pass(n_src):
    """late queries one pass of a pair's workgroups takes: four rows a workgroup (associate_fit_late_kernel)"""
    return S.rest_blocks_one_pair(n_src) * 4


def list_length(late, n_src=48):
    """the wall, `late` queries on it and n_src - late far away: rows_per_pass(48) = 16"""
    rng = np.random.default_rng(201)
    tgt = S.wall_points(rng, 2000)
    on = tgt[rng.choice(len(tgt), late, replace=False)] + rng.normal(size=(late, 3)) * 0.01
    src = np.concatenate([on, FAR + rng.uniform(-1, 1, (n_src - late, 3))])
    se, te = S.edge_pair(rng)
    return S.scene("late_%d_of_%d" % (late, n_src), "plane", se, src, te, tgt), late


def filler(rng, n=520):
    """a second cluster 60 m away (the planar set stays above kBruteMax) and the outliers that make the box 100 m wide"""
    return np.concatenate([rng.uniform(-0.05, 0.05, (n, 3)) + np.array([-30.0, 28.0, -25.0]), OUTLIERS])


def block_population(m, k=5, n_q=24):
    """m points in a cube of 0.1 m, alone in their 3x3x3 block: a late query's row deals exactly m candidates (m < k: kept < k;
    15 / 16 / 17 / 33: a lane short, every lane one, one lane a second, two batches' worth of lanes uneven; 244 - 252: sixteen a lane,
    the trip_budget scenes' cell). n_q queries inside the cube; all of them are finished by round 1"""
    rng = np.random.default_rng(202 + m)
    a = rng.uniform(-0.05, 0.05, (m, 3)) + A
    src = A + rng.uniform(-0.05, 0.05, (n_q, 3))
    se, te = S.edge_pair(rng)
    return S.scene("block_%d_k%d" % (m, k), "plane", se, src, te, np.concatenate([a, filler(rng)]), k_p=k), n_q


def empty_block(n_q=8):
    """queries 20 m from every point, inside the box: their 3x3x3 blocks (4.4 m cells) are empty. Nothing is nearer than the
    block's faces, which are farther than the radius: round 1 finishes them with no neighbour at all"""
    rng = np.random.default_rng(203)
    src = np.array([20.0, 20.0, -20.0]) + rng.uniform(-0.5, 0.5, (n_q, 3))
    se, te = S.edge_pair(rng)
    return S.scene("block_0", "plane", se, src, te, np.concatenate([rng.uniform(-0.05, 0.05, (40, 3)) + A, filler(rng)])), n_q


def over_capacity(h, n_q=24):
    """two clusters of 150 points on either side of a cell face (y): 300 candidates in the block of a query next to the face —
    more than the row's 256 — in rows of 150. The queries sit in the middle of the lower cluster, 0.07 m or more from the face
    and 0.03 m from their fifth neighbour: round 1 leaves the other row out once its bound is below the face's distance (38
    batches: within the 64-trip budget that would otherwise queue the query wide) and finishes them. The row deals the block as
    it stands, refuses it, and lane 0 searches alone. `h`: the grid's cell edge (the face is placed from it, and the caller
    checks the scene against the grid it gets)"""
    rng = np.random.default_rng(204)
    face = -50.0 + np.ceil((A[1] + 50.0) / h) * h  # the first cell face above A's y
    lo = np.array([A[0], face - 0.1, A[2]]) + rng.uniform(-0.05, 0.05, (150, 3))
    hi = np.array([A[0], face + 0.06, A[2]]) + rng.uniform(-0.05, 0.05, (150, 3))
    src = np.array([A[0], face - 0.1, A[2]]) + rng.uniform(-0.03, 0.03, (n_q, 3))
    se, te = S.edge_pair(rng)
    return S.scene("over_capacity", "plane", se, src, te, np.concatenate([lo, hi, filler(rng)])), n_q


def radius_shells(k):
    """six queries 8 m apart, each with five points around it at 2 m (1 +- (1 + u) 1e-9), u = 0 .. 4 — distinct distances, nine
    decimal places from the radius — of which the j nearest, j = 0 .. 5, are inside: kept = min(j, k). 1e-9 is seven orders above
    the rounding of a squared distance and far below what the FP32 keys resolve: the radius filter is the exact search's"""
    rng = np.random.default_rng(205)
    src, tgt = [], []
    for j in range(6):
        q = A + np.array([8.0 * j, 0.0, 0.0])
        src.append(q)
        for u in range(5):
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            tgt.append(q + d * 2.0 * (1.0 - (1 + u) * 1e-9 if u < j else 1.0 + (1 + u) * 1e-9))
    se, te = S.edge_pair(rng)
    return S.scene("radius_k%d" % k, "plane", se, np.array(src), te, np.concatenate([np.array(tgt), filler(rng)]), k_p=k), 6


def kept_of_radius_shells(k):
    return [min(j, k) for j in range(6)]


def box_edges():
    """3 000 uniform points in a 4 m cube (h = r / 4 = 0.5: 9^3 cells, ~4 points a cell, ~110 a block, the fifth neighbour ~0.2 m
    away) and queries 0.37 h into the eight corner cells, into the cells one outside the grid on each of the six sides, and one
    outside along the diagonals: round 1 searches all of them (out <= 1) with rows and cells clamped at the grid's edges"""
    rng = np.random.default_rng(206)
    tgt = rng.uniform(0.0, 4.0, (3000, 3))
    origin, h, dims = S.grid_of(tgt, 2.0)
    cells = []
    for cx in (0, dims[0] - 1):
        for cy in (0, dims[1] - 1):
            for cz in (0, dims[2] - 1):
                cells.append((cx, cy, cz))
                cells.append((cx + (-1 if cx == 0 else 1), cy + (-1 if cy == 0 else 1), cz + (-1 if cz == 0 else 1)))
    for axis in range(3):
        for side in (-1, 1):
            for rep in range(3):
                c = rng.integers(1, dims - 1)
                c[axis] = -1 if side < 0 else dims[axis]
                cells.append(tuple(c))
    src = origin + (np.array(cells, dtype=np.float64) + 0.37) * h
    se, te = S.edge_pair(rng)
    return S.scene("box_edges", "plane", se, src, te, tgt), S.cell_out(src, origin, h, dims)


def flat(n_q=60):
    """2 000 points EXACTLY on the plane y = 5 (ny = 1: a grid one cell deep, no rows above or below) and queries a centimetre
    off it on either side: half of them in the grid's only layer, half one cell outside it"""
    rng = np.random.default_rng(207)
    tgt = S.wall_points(rng, 2000)
    tgt[:, 1] = 5.0
    src = tgt[rng.choice(2000, n_q, replace=False)] + rng.normal(size=(n_q, 3)) * 0.01
    src[:, 1] = 5.0 + np.where(np.arange(n_q) % 2 == 0, 0.01, -0.01)
    se, te = S.edge_pair(rng)
    return S.scene("flat", "plane", se, src, te, tgt), n_q


def duplicates(n_q=60):
    """the wall's first 1 000 points twice over: every neighbour has a twin at exactly its distance, which only the original index
    orders (ties: the oracle's tree has its own order among equals)"""
    rng = np.random.default_rng(208)
    half = S.wall_points(rng, 1000)
    tgt = np.concatenate([half, half])
    src = half[rng.choice(1000, n_q, replace=False)] + rng.normal(size=(n_q, 3)) * 0.01
    se, te = S.edge_pair(rng)
    return S.scene("duplicates", "plane", se, src, te, tgt, ties=True), n_q
