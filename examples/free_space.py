#!/usr/bin/env python3
"""Free space: the drive of examples/global_map.py with an occupancy map filled beside the cloud map.

    python -m loam_amd.build            # once: libloamx.so + the pybind11 module
    python examples/free_space.py [--leaf 0.2]

The scans of the drive are registered, the trajectory is corrected by the pose graph and the scans are motion-corrected on the
device, exactly as examples/global_map.py does it. At the corrected poses the cloud map and the occupancy map then take the
same call on the same device buffers (`add_clouds_dev` of both: neither the scans nor the poses visit the host). The cloud
map's centroids are handed to the occupancy map's `query_dev` where `emit_dev` left them, and the program prints the share of
them that lies in an OCCUPIED voxel, the map's counters, and a coarse picture of the slice at sensor height:
`#` occupied, `.` free, blank unknown."""
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
REACH = 45.0  # metres around the drive that the slice shows


def picture(grid, cell):
    """one character per cell x cell block of the slice: occupied wins over free wins over unknown; north is up"""
    h, w = (grid.shape[0] // cell) * cell, (grid.shape[1] // cell) * cell
    blocks = grid[:h, :w].reshape(h // cell, cell, w // cell, cell).max(axis=(1, 3))
    return "\n".join("".join(" .#"[v] for v in row) for row in blocks[::-1])


def main(scan_lines=32, points_per_line=512, leaf=0.2, max_voxels=1 << 18, max_free_voxels=1 << 23, verbose=True, ctx=None):
    from loam_amd import capi
    c = ctx or capi.Context(0)
    H, W, n = scan_lines, points_per_line, N_SCANS
    lidar = capi.LidarParams(H, W, 1.0, 120.0)
    motions = np.tile(IDENTITY, (n, 1))
    offsets = np.arange(n + 1) * (H * W)
    params = capi.OccupancyParams(leaf=leaf)
    bufs, out = [], {}

    def room(nbytes):
        bufs.append(c.alloc(nbytes))
        return bufs[-1]

    cloud_map = c.cloud_map(capi.CloudMapParams(leaf=leaf, max_range=params.max_range), max_voxels)
    free_space = c.occupancy_map(params, max_free_voxels)

    def fill(stage, c, d_scans, d_traj):
        """at the corrected poses; everything up to the downloads is enqueued behind the solve that made d_traj"""
        if stage != "corrected":
            return
        d_deskewed, d_motions = room(n * H * W * 3 * 4), room(motions.nbytes).upload(motions)
        d_xyz, d_n, d_counts, d_states = room(max_voxels * 24), room(4), room(max_voxels * 8), room(max_voxels)
        c.deskew_scans_dev(d_scans.ptr, n, lidar, d_motions.ptr, d_deskewed.ptr, ref_fraction=1.0, f32=True)
        cloud_map.add_clouds_dev(d_deskewed.ptr, 3, offsets, d_traj.ptr, f32=True)
        free_space.add_clouds_dev(d_deskewed.ptr, 3, offsets, d_traj.ptr, f32=True)
        cloud_map.emit_dev(d_xyz.ptr, max_voxels, d_n.ptr)
        free_space.query_dev(d_xyz.ptr, 3, max_voxels, d_counts.ptr, d_states.ptr)  # (what lies behind the centroids is not looked at below)
        m = int(d_n.download(np.uint32, 1)[0])
        out["centroids"] = d_xyz.download(np.float64, 3 * m).reshape(-1, 3)
        out["centroid_counts"] = d_counts.download(np.uint32, 2 * m).reshape(-1, 2)
        out["centroid_states"] = d_states.download(np.uint8, m)
        out["poses"] = d_traj.download(np.float64, n * 7).reshape(n, 7)
        out["deskewed"] = d_deskewed.download(np.float32, n * H * W * 3).reshape(n, H * W, 3)
        out["stats"], out["cloud_stats"] = free_space.stats(), cloud_map.stats()
        # the slice at sensor height: three levels around the first pose's, REACH metres around the drive
        t = out["poses"][:, 4:]
        lo, hi = np.floor((t.min(axis=0) - REACH) / leaf), np.floor((t.max(axis=0) + REACH) / leaf)
        level = np.floor(t[0, 2] / leaf)
        out["slice_vmin"] = np.array([lo[0], lo[1], level - 1], dtype=np.int32)
        out["slice_dims"] = np.array([hi[0] - lo[0] + 1, hi[1] - lo[1] + 1, 3], dtype=np.uint32)
        out["slice"] = free_space.slice(out["slice_vmin"], out["slice_dims"])

    try:
        drive = pose_graph.main(scan_lines=H, points_per_line=W, verbose=False, ctx=c, stage_hook=fill)
    finally:
        cloud_map.close(), free_space.close()
        for b in bufs:
            b.free()

    out["occupied_share"] = float((out["centroid_states"] == capi.OCC_OCCUPIED).mean())
    out["params"] = {k: getattr(params, k) for k in params.NAMES}
    out["drive"] = drive
    if verbose:
        st = out["stats"]
        print("%d scans of %d x %d points, leaf %.2f m" % (n, H, W, leaf))
        print("  occupancy map: " + "  ".join("%s %d" % (k, int(st[k])) for k in capi.OCCUPANCY_STATS_DTYPE.names))
        print("  %d centroids of the cloud map, %.1f %% of them in an OCCUPIED voxel" % (len(out["centroids"]), 100.0 * out["occupied_share"]))
        grid = out["slice"]
        print("  slice at sensor height, %d x %d cells: %d occupied, %d free, %d unknown" % (
            grid.shape[1], grid.shape[0], (grid == capi.OCC_OCCUPIED).sum(), (grid == capi.OCC_FREE).sum(), (grid == capi.OCC_UNKNOWN).sum()))
        print(picture(grid, max(1, grid.shape[1] // 100)))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--leaf", type=float, default=0.2, help="voxel edge in metres")
    args = ap.parse_args()
    main(leaf=args.leaf)
