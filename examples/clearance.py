#!/usr/bin/env python3
"""Clearance: the drive of examples/free_space.py with the occupancy map's slice turned into a distance field on the device.

    python -m loam_amd.build            # once: libloamx.so + the pybind11 module
    python examples/clearance.py [--leaf 0.2] [--radius 0.6]

The scans of the drive are registered, corrected by the pose graph and motion-corrected on the device, and the occupancy map takes
them at the corrected poses, exactly as examples/free_space.py does it. The slice at sensor height then becomes a clearance grid
(`distance_slice_dev`: per cell the exact distance to the nearest OCCUPIED cell, the map read in a halo around the grid), enqueued
behind the add without a host copy in between. The program prints the share of FREE cells that lie nearer to an obstacle than a
robot radius, and a coarse picture of the grid with the obstacles inflated by that radius:
`#` occupied, `+` free but within the radius, `.` free with clearance, blank unknown."""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

_spec = importlib.util.spec_from_file_location("pose_graph_drive", os.path.join(os.path.dirname(os.path.abspath(__file__)), "pose_graph.py"))
pose_graph = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pose_graph)

N_SCANS = pose_graph.N_SCANS
IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
REACH = 45.0  # metres around the drive that the grid shows


def picture(cells, cell):
    """one character per cell x cell block: the largest class of the block wins (occupied > inflated > free > unknown); north is up"""
    h, w = (cells.shape[0] // cell) * cell, (cells.shape[1] // cell) * cell
    blocks = cells[:h, :w].reshape(h // cell, cell, w // cell, cell).max(axis=(1, 3))
    return "\n".join("".join(" .+#"[v] for v in row) for row in blocks[::-1])


def main(scan_lines=32, points_per_line=512, leaf=0.2, radius=0.6, max_free_voxels=1 << 23, verbose=True, ctx=None):
    from loam_amd import capi
    c = ctx or capi.Context(0)
    H, W, n = scan_lines, points_per_line, N_SCANS
    lidar = capi.LidarParams(H, W, 1.0, 120.0)
    motions = np.tile(IDENTITY, (n, 1))
    offsets = np.arange(n + 1) * (H * W)
    params = capi.OccupancyParams(leaf=leaf)
    reach_voxels = int(np.ceil(radius / leaf)) + 2  # the cap: a little beyond the radius is all the inflation needs
    dist = capi.DistanceParams(max_dist_voxels=reach_voxels)
    bufs, out = [], {}

    def room(nbytes):
        bufs.append(c.alloc(nbytes))
        return bufs[-1]

    free_space = c.occupancy_map(params, max_free_voxels)

    def fill(stage, c, d_scans, d_traj):
        if stage != "corrected":
            return
        d_deskewed, d_motions = room(n * H * W * 3 * 4), room(motions.nbytes).upload(motions)
        c.deskew_scans_dev(d_scans.ptr, n, lidar, d_motions.ptr, d_deskewed.ptr, ref_fraction=1.0, f32=True)
        free_space.add_clouds_dev(d_deskewed.ptr, 3, offsets, d_traj.ptr, f32=True)
        out["poses"] = d_traj.download(np.float64, n * 7).reshape(n, 7)  # (the grid's place comes from the poses)
        t = out["poses"][:, 4:]
        lo, hi = np.floor((t.min(axis=0) - REACH) / leaf), np.floor((t.max(axis=0) + REACH) / leaf)
        level = np.floor(t[0, 2] / leaf)
        vmin = np.array([lo[0], lo[1], level - 1], dtype=np.int32)
        dims = np.array([hi[0] - lo[0] + 1, hi[1] - lo[1] + 1, 3], dtype=np.uint32)
        cells = int(dims[0]) * int(dims[1])
        d_grid, d_d2, d_off, d_m = room(cells), room(cells * 2), room(cells * 4), room(cells * 4)
        free_space.slice_dev(vmin, dims, d_grid.ptr)
        free_space.distance_slice_dev(vmin, dims, dist, d_d2.ptr, d_off.ptr, d_m.ptr)
        shape = (int(dims[1]), int(dims[0]))
        out["slice_vmin"], out["slice_dims"] = vmin, dims
        out["slice"] = d_grid.download(np.uint8, cells).reshape(shape)
        out["d2"] = d_d2.download(np.uint16, cells).reshape(shape)
        out["offset"] = d_off.download(np.int16, cells * 2).reshape(shape + (2,))
        out["metres"] = d_m.download(np.float32, cells).reshape(shape)
        out["stats"] = free_space.stats()

    try:
        drive = pose_graph.main(scan_lines=H, points_per_line=W, verbose=False, ctx=c, stage_hook=fill)
    finally:
        free_space.close()
        for b in bufs:
            b.free()

    grid, metres = out["slice"], out["metres"]
    free = grid == capi.OCC_FREE
    tight = free & (metres < radius)
    out["free_cells"], out["tight_cells"] = int(free.sum()), int(tight.sum())
    out["tight_share"] = float(tight.sum()) / max(1, int(free.sum()))
    out["radius"], out["max_dist_voxels"], out["leaf"] = radius, reach_voxels, leaf
    out["classes"] = np.where(grid == capi.OCC_OCCUPIED, 3, np.where(tight, 2, np.where(free, 1, 0))).astype(np.uint8)
    out["drive"] = drive
    if verbose:
        print("%d scans of %d x %d points, leaf %.2f m, robot radius %.2f m (cap %d voxels)" % (n, H, W, leaf, radius, reach_voxels))
        print("  clearance grid at sensor height, %d x %d cells: %d occupied, %d free, %d unknown" % (
            grid.shape[1], grid.shape[0], (grid == capi.OCC_OCCUPIED).sum(), free.sum(), (grid == capi.OCC_UNKNOWN).sum()))
        print("  %.1f %% of the FREE cells are nearer than %.2f m to an obstacle" % (100.0 * out["tight_share"], radius))
        print(picture(out["classes"], max(1, grid.shape[1] // 100)))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--leaf", type=float, default=0.2, help="voxel edge in metres")
    ap.add_argument("--radius", type=float, default=0.6, help="robot radius in metres")
    args = ap.parse_args()
    main(leaf=args.leaf, radius=args.radius)
