#!/usr/bin/env python3
"""Surface normals of the map: the drive of examples/global_map.py assembled into a surfel map at the corrected poses.

    python -m loam_amd.build            # once: libloamx.so + the pybind11 module
    python examples/surface_normals.py [--leaf 1.0]

The scans of the drive are registered as a sequence, the trajectory is composed on the device and corrected by the pose graph
with its one loop edge (examples/pose_graph.py). Right behind the solve, before anything synchronises, the scans go into a
surfel map at the corrected poses read from the trajectory buffer on the device (`add_clouds_dev`), and the map's records are
emitted (`emit_dev`). The program prints
  - the share of voxels that are flat: eval[0] / eval[2] under a bound,
  - the mean angle of the ground voxels' normals to +z,
  - the mean absolute distance of the last scan's points to the surfels of their voxels (`query`)."""
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
FLATNESS = 0.02    # a voxel is flat when its smallest eigenvalue is under this share of its largest
MIN_POINTS = 8     # voxels with fewer points say little about a surface
GROUND_Z = 0.15    # a voxel whose mean lies this close to z = 0 is ground


def act(pose, p):
    """pose.act(p) for (n, 3) points: rotation by the unit quaternion (x y z w), then the translation"""
    u, w = pose[:3], pose[3]
    uv = 2.0 * np.cross(u, p)
    return p + w * uv + np.cross(u, uv) + pose[4:]


def main(scan_lines=32, points_per_line=512, leaf=1.0, max_voxels=1 << 17, verbose=True, ctx=None):
    from loam_amd import capi
    c = ctx or capi.Context(0)
    H, W, n = scan_lines, points_per_line, N_SCANS
    offsets = np.arange(n + 1) * (H * W)
    bufs, out = [], {}

    def room(nbytes):
        bufs.append(c.alloc(nbytes))
        return bufs[-1]

    surfel_map = c.surfel_map(capi.SurfelMapParams(leaf=leaf), max_voxels)

    def assemble(stage, c, d_scans, d_traj):
        """enqueued right behind the solve; the downloads at the end are the first synchronisation"""
        if stage != "corrected":
            return
        d_rec, d_n = room(max_voxels * capi.SURFEL_DTYPE.itemsize), room(4)
        surfel_map.add_clouds_dev(d_scans.ptr, 3, offsets, d_traj.ptr, f32=True)
        surfel_map.emit_dev(max_voxels, d_n.ptr, MIN_POINTS, d_out=d_rec.ptr)
        out["voxels"] = int(d_n.download(np.uint32, 1)[0])
        out["surfels"] = d_rec.download(capi.SURFEL_DTYPE, out["voxels"])
        out["stats"] = surfel_map.stats()
        out["poses"] = d_traj.download(np.float64, n * 7).reshape(n, 7)
        out["scans"] = d_scans.download(np.float32, n * H * W * 3).reshape(n, H * W, 3)
        out["last_scan"] = out["scans"][-1].astype(np.float64)

    try:
        drive = pose_graph.main(scan_lines=H, points_per_line=W, verbose=False, ctx=c, stage_hook=assemble)
        # the last scan against the map it is part of: its points at their corrected pose
        hit = (out["last_scan"] != 0.0).any(axis=1)
        world = act(out["poses"][-1], out["last_scan"][hit])
        rec, dist, count = surfel_map.query(world, MIN_POINTS)
    finally:
        surfel_map.close()
        for b in bufs:
            b.free()

    s = out["surfels"]
    flat = s["eval"][:, 0] <= FLATNESS * s["eval"][:, 2]
    ground = flat & (np.abs(s["mean"][:, 2]) < GROUND_Z)
    angle = np.degrees(np.arccos(np.clip(s["normal"][ground, 2], -1.0, 1.0)))
    found = count > 0
    out.update(flat_share=float(flat.mean()), ground_voxels=int(ground.sum()), ground_angle_deg=float(angle.mean()) if ground.any() else float("nan"),
               queried=int(hit.sum()), found=int(found.sum()), mean_abs_distance=float(np.abs(dist[found]).mean()) if found.any() else float("nan"),
               leaf=leaf, drive=drive, query_records=rec, query_distance=dist, query_count=count, query_points=world)
    if verbose:
        st = out["stats"]
        print("%d scans of %d x %d points, leaf %.2f m: %d voxels, %d with at least %d points" % (n, H, W, leaf, int(st["voxels"]), out["voxels"], MIN_POINTS))
        print("  flat (eval[0] / eval[2] <= %.2f): %.1f %% of them" % (FLATNESS, 100.0 * out["flat_share"]))
        print("  ground: %d voxels, normals %.2f degrees from +z on average" % (out["ground_voxels"], out["ground_angle_deg"]))
        print("  last scan: %d of %d points lie in such a voxel, %.3f m from its plane on average" % (out["found"], out["queried"], out["mean_abs_distance"]))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--leaf", type=float, default=1.0, help="voxel edge in metres")
    args = ap.parse_args()
    main(leaf=args.leaf)
