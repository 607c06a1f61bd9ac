#!/usr/bin/env python3
"""The scan the map expects: the drive of examples/free_space.py, one scan held out, and that scan rendered from the map.

    python -m loam_amd.build            # once: libloamx.so + the pybind11 module
    python examples/expected_scan.py [--leaf 0.2]

The scans of the drive are registered, the trajectory is corrected by the pose graph and the scans are motion-corrected on the
device, as examples/free_space.py does it. The occupancy map then takes every scan but one at its corrected pose, and
`render_scans_dev` casts the beams of the sensor (`capi.beam_directions`: the centres of the scan's cells) through the map at the
pose of the scan that was held out. The program prints the share of beams whose measured range and the range the map predicts
agree within one leaf, and the same share after the pose is moved 1 m sideways: the independent check of a pose that a
localiser's own convergence flag is not. A predicted range is the middle of a voxel, so it is quantised to the leaf.

Over ALL beams the share is low even at the right pose, and that is the voxel grid, not the pose: most beams of this sensor meet
the ground at a grazing angle, and a beam that comes down at 5 degrees runs inside the top layer of OCCUPIED ground voxels for
leaf / tan(5 degrees), two metres and more, before it reaches its own return, so the map stops it early. The share that tells
poses apart is that of the beams whose return stands clear of the ground (walls, vehicles); the program prints both, and the
share at a tolerance of two leaves."""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)
import outdoor_scenes  # noqa: E402  (only for the fan of the stand-in sensor)

_spec = importlib.util.spec_from_file_location("pose_graph_drive", os.path.join(os.path.dirname(os.path.abspath(__file__)), "pose_graph.py"))
pose_graph = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pose_graph)

N_SCANS = pose_graph.N_SCANS
IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


def sideways(pose, metres):
    """the pose moved along its own y axis"""
    x, y, z, w = pose[:4]
    left = np.array([2 * (x * y - w * z), 1 - 2 * (x * x + z * z), 2 * (y * z + w * x)])
    return np.concatenate([pose[:4], pose[4:] + metres * left])


RAISED = 0.5  # metres above the ground from which a return counts as standing clear of it


def rotate(pose, p):
    """the rotation of a pose (qx qy qz qw ...) on (n, 3) points"""
    u, w = pose[:3], pose[3]
    uv = 2.0 * np.cross(u, p)
    return p + w * uv + np.cross(u, uv)


def agreement(measured, predicted, tolerance, among=None):
    """(share of the beams with a return in both scans, and in `among`, whose ranges agree within the tolerance; how many those are)"""
    both = (measured > 0) & (predicted > 0)
    if among is not None:
        both &= among
    return (float((np.abs(measured - predicted)[both] <= tolerance).mean()) if both.any() else 0.0), int(both.sum())


def main(scan_lines=32, points_per_line=512, leaf=0.2, max_voxels=1 << 23, held_out=None, verbose=True, ctx=None):
    from loam_amd import capi
    c = ctx or capi.Context(0)
    H, W, n = scan_lines, points_per_line, N_SCANS
    k = n // 2 if held_out is None else int(held_out)
    lidar = capi.LidarParams(H, W, 1.0, 120.0)
    motions = np.tile(IDENTITY, (n, 1))
    offsets = np.arange(n + 1) * (H * W)
    params = capi.OccupancyParams(leaf=leaf)
    top, bottom = outdoor_scenes.FANS["lot"]
    dirs = capi.beam_directions(H, W, capi.OrganizeParams(fov_bottom=np.radians(bottom), fov_top=np.radians(top)))
    bufs, out = [], {}

    def room(nbytes):
        bufs.append(c.alloc(nbytes))
        return bufs[-1]

    free_space = c.occupancy_map(params, max_voxels)

    def fill(stage, c, d_scans, d_traj):
        """at the corrected poses; everything up to the downloads is enqueued behind the solve that made d_traj"""
        if stage != "corrected":
            return
        d_deskewed, d_motions = room(n * H * W * 3 * 4), room(motions.nbytes).upload(motions)
        d_dirs, d_poses, d_ranges = room(dirs.nbytes).upload(dirs), room(2 * 7 * 8), room(2 * H * W * 8)
        c.deskew_scans_dev(d_scans.ptr, n, lidar, d_motions.ptr, d_deskewed.ptr, ref_fraction=1.0, f32=True)
        # every scan but scan k: the clouds in front of it and the clouds behind it, each with its poses
        free_space.add_clouds_dev(d_deskewed.ptr, 3, offsets[:k + 1], d_traj.ptr, f32=True)
        free_space.add_clouds_dev(d_deskewed.ptr, 3, offsets[k + 1:], d_traj.ptr + (k + 1) * 7 * 8, f32=True)
        out["poses"] = d_traj.download(np.float64, n * 7).reshape(n, 7)
        out["render_poses"] = np.stack([out["poses"][k], sideways(out["poses"][k], 1.0)])
        d_poses.upload(out["render_poses"])
        free_space.render_scans_dev(d_dirs.ptr, H * W, d_poses.ptr, 2, params.max_range, d_ranges_out=d_ranges.ptr)
        out["predicted"] = d_ranges.download(np.float64, 2 * H * W).reshape(2, H * W)
        out["census"] = c.last_raycast_census()
        scan = d_deskewed.download(np.float32, n * H * W * 3).reshape(n, H * W, 3)[k].astype(np.float64)
        out["measured"] = np.sqrt((scan * scan).sum(axis=1))
        out["height"] = rotate(out["poses"][k], scan)[:, 2] + out["poses"][k][6]  # of every return above the ground plane z = 0
        out["stats"] = free_space.stats()

    try:
        out["drive"] = pose_graph.main(scan_lines=H, points_per_line=W, verbose=False, ctx=c, stage_hook=fill)
    finally:
        free_space.close()
        for b in bufs:
            b.free()

    out["held_out"], out["leaf"] = k, leaf
    raised = out["height"] > RAISED
    for name, i in (("", 0), ("_moved", 1)):
        out["agree" + name], out["beams" + name] = agreement(out["measured"], out["predicted"][i], leaf)
        out["agree_two_leaves" + name], _ = agreement(out["measured"], out["predicted"][i], 2 * leaf)
        out["agree_raised" + name], out["beams_raised" + name] = agreement(out["measured"], out["predicted"][i], leaf, raised)
    if verbose:
        cen = out["census"]
        print("%d scans of %d x %d points, leaf %.2f m; scan %d held out, %d voxels in the map" % (n, H, W, leaf, k, int(out["stats"]["voxels"])))
        print("  rendered 2 x %d beams: %d hit, %d clear, %d truncated; %d visits in %d look-ups" % (
            H * W, int(cen["hit"]), int(cen["clear"]), int(cen["truncated"]), int(cen["visits"]), int(cen["probes"])))
        for name, what in (("", "at the scan's own pose"), ("_moved", "moved 1 m sideways    ")):
            print("  %s: %5.1f %% of the %d beams whose return stands %.1f m clear of the ground agree with the map within one leaf" % (
                what, 100.0 * out["agree_raised" + name], out["beams_raised" + name], RAISED))
            print("  %s  %5.1f %% of all %d beams (%.1f %% within two leaves): beams that graze the ground stop early in its voxels" % (
                " " * len(what), 100.0 * out["agree" + name], out["beams" + name], 100.0 * out["agree_two_leaves" + name]))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--leaf", type=float, default=0.2, help="voxel edge in metres")
    args = ap.parse_args()
    main(leaf=args.leaf)
