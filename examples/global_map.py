#!/usr/bin/env python3
"""The map: the drive of examples/pose_graph.py assembled into a centroid voxel grid, before and after the loop closure.

    python -m loam_amd.build            # once: libloamx.so + the pybind11 module
    python examples/global_map.py [--leaf 0.2]

The scans of the drive are registered as a sequence, the trajectory is composed on the device and corrected by the pose graph
with its one loop edge, exactly as examples/pose_graph.py does it. The scans are motion-corrected on the device
(`deskew_scans_dev`) and assembled into a cloud map twice: once at the odometry poses, and once, after `clear`, at the
corrected poses read straight from the trajectory buffer the solve left on the device (`add_clouds_dev`: the poses never
visit the host). The program prints both voxel counts and both sets of counters.

The stand-in scans are ray casts from standing poses, so the motion handed to the de-skew is the identity; a vehicle passes
its previous step there, as examples/scan_sequence.py does."""
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


def main(scan_lines=32, points_per_line=512, leaf=0.2, max_voxels=1 << 18, verbose=True, ctx=None):
    from loam_amd import capi
    c = ctx or capi.Context(0)
    H, W, n = scan_lines, points_per_line, N_SCANS
    lidar = capi.LidarParams(H, W, 1.0, 120.0)
    motions = np.tile(IDENTITY, (n, 1))
    offsets = np.arange(n + 1) * (H * W)
    bufs, out = [], {}

    def room(nbytes):
        bufs.append(c.alloc(nbytes))
        return bufs[-1]

    cloud_map = c.cloud_map(capi.CloudMapParams(leaf=leaf), max_voxels)

    def assemble(stage, c, d_scans, d_traj):
        """everything here is enqueued behind what made d_traj; the downloads at the end are the first synchronisation"""
        if stage == "odometry":
            out["d_deskewed"], d_motions = room(n * H * W * 3 * 4), room(motions.nbytes).upload(motions)
            out["d_xyz"], out["d_n"] = room(max_voxels * 24), room(4)
            c.deskew_scans_dev(d_scans.ptr, n, lidar, d_motions.ptr, out["d_deskewed"].ptr, ref_fraction=1.0, f32=True)
        else:
            cloud_map.clear()
        cloud_map.add_clouds_dev(out["d_deskewed"].ptr, 3, offsets, d_traj.ptr, f32=True)
        cloud_map.emit_dev(out["d_xyz"].ptr, max_voxels, out["d_n"].ptr)
        out[stage + "_stats"] = cloud_map.stats()
        out[stage + "_voxels"] = int(out["d_n"].download(np.uint32, 1)[0])
        out[stage + "_cloud"] = out["d_xyz"].download(np.float64, 3 * out[stage + "_voxels"]).reshape(-1, 3)
        out[stage + "_poses"] = d_traj.download(np.float64, n * 7).reshape(n, 7)

    try:
        # the drive of examples/pose_graph.py: sequence, trajectory, loop edge, solve; the maps are assembled at its two stages
        drive = pose_graph.main(scan_lines=H, points_per_line=W, verbose=False, ctx=c, stage_hook=assemble)
        out["deskewed"] = out["d_deskewed"].download(np.float32, n * H * W * 3).reshape(n, H * W, 3)
    finally:
        cloud_map.close()
        for b in bufs:
            b.free()

    if verbose:
        names = capi.CLOUD_MAP_STATS_DTYPE.names
        print("%d scans of %d x %d points, leaf %.2f m" % (n, H, W, leaf))
        for stage in ("odometry", "corrected"):
            st = out[stage + "_stats"]
            print("  %-9s poses: %7d voxels   " % (stage, out[stage + "_voxels"]) + "  ".join("%s %d" % (k, int(st[k])) for k in names[1:]))
        print("last pose: %.3f m from the truth before the optimisation, %.3f m after" % (drive["before"], drive["after"]))
    result = {k: v for k, v in out.items() if not k.startswith("d_")}
    result.update(leaf=leaf, drive=drive)
    return result


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--leaf", type=float, default=0.2, help="voxel edge in metres")
    args = ap.parse_args()
    main(leaf=args.leaf)
