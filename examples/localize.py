#!/usr/bin/env python3
"""Scan-to-map localisation: the second lap of a drive placed on the surfel map of the first.

    python -m loam_amd.build            # once: libloamx.so + the pybind11 module
    python examples/localize.py [--leaf 0.5]

The drive is the circle in the lot of examples/loop_closure.py (and so of examples/surface_normals.py). The scans of the first lap
go into a surfel map at their poses. The second lap runs the same circle half a step further on and 0.2 m wider; each of its scans
starts from an odometry pose (the true pose off by 0.15 m and 1 degree, fixed seed) and is placed on the map by
`SurfelMap.localize`: point-to-plane Gauss-Newton against the voxels' fitted planes, solved on the device. The program prints, per
scan, the distance to the true pose before and after, the iterations, and the smallest eigenvalue of the information matrix per
row (small where the map leaves a direction open)."""
import argparse
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
sys.path.insert(0, ROOT)

_spec = importlib.util.spec_from_file_location("loop_closure_drive", os.path.join(HERE, "loop_closure.py"))
loop_closure = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(loop_closure)
outdoor_scenes = loop_closure.outdoor_scenes

N_FIRST_LAP = loop_closure.N_SCANS - 1  # the circle without the revisit at its end
N_SECOND_LAP = 8


def second_lap(n=N_SECOND_LAP):
    """[(position, heading)]: the circle of the first lap, half a step further on and 0.2 m wider"""
    o0, yaw0 = outdoor_scenes.sensor_origin("lot", 0)
    centre = o0 - 3.5 * np.array([np.cos(yaw0 + np.pi / 2), np.sin(yaw0 + np.pi / 2), 0.0])
    poses = []
    for i in range(n):
        a = 2.0 * np.pi * (i + 0.5) / N_FIRST_LAP
        poses.append((centre + 3.7 * np.array([np.cos(yaw0 + np.pi / 2 + a), np.sin(yaw0 + np.pi / 2 + a), 0.0]), yaw0 + a))
    return poses


def odometry(pose7, seed, metres=0.15, degrees=1.0):
    """the true pose off by a step of that size in the sensor's own frame"""
    rng = np.random.default_rng([17, seed])
    axis, t = rng.normal(size=3), rng.normal(size=3)
    axis, t = axis / np.linalg.norm(axis), t / np.linalg.norm(t) * metres
    half = np.radians(degrees) / 2.0
    import loam
    true = loam.Pose3d(loam.Quaterniond(pose7[3], pose7[0], pose7[1], pose7[2]), pose7[4:])
    step = loam.Pose3d(loam.Quaterniond(np.cos(half), *(np.sin(half) * axis)), t)
    return true, true.compose(step)


def main(scan_lines=32, points_per_line=512, leaf=0.5, verbose=True):
    import loam
    H, W = scan_lines, points_per_line
    params = loam.SurfelMapParams()
    params.leaf = leaf
    surfel_map = loam.SurfelMap(params, 1 << 17)
    for i, (origin, yaw) in enumerate(loop_closure.drive()[:N_FIRST_LAP]):
        scan = np.ascontiguousarray(outdoor_scenes.scan_at("lot", 0, origin, yaw, H, W, noise_seed=i), dtype=np.float32)
        p7 = outdoor_scenes.yaw_pose(yaw, origin)
        surfel_map.add(scan, loam.Pose3d(loam.Quaterniond(p7[3], p7[0], p7[1], p7[2]), p7[4:]))
    out = dict(before=[], after=[], iterations=[], termination=[], smallest_eigenvalue=[], rows=[], voxels=surfel_map.stats()["voxels"])
    for i, (origin, yaw) in enumerate(second_lap()):
        scan = np.ascontiguousarray(outdoor_scenes.scan_at("lot", 0, origin, yaw, H, W, noise_seed=100 + i), dtype=np.float32)
        true, start = odometry(outdoor_scenes.yaw_pose(yaw, origin), i)
        pose, result, information = surfel_map.localize(scan, start)
        out["before"].append(float(np.linalg.norm(np.asarray(start.translation) - np.asarray(true.translation))))
        out["after"].append(float(np.linalg.norm(np.asarray(pose.translation) - np.asarray(true.translation))))
        out["iterations"].append(int(result.iterations)), out["termination"].append(int(result.termination)), out["rows"].append(int(result.n_rows))
        out["smallest_eigenvalue"].append(float(information.eigenvalues.reshape(-1)[0]) / max(int(result.n_rows), 1))
    if verbose:
        print("map of %d scans of %d x %d points at leaf %.2f m: %d voxels" % (N_FIRST_LAP, H, W, leaf, out["voxels"]))
        print("scan   before   after   iterations   rows   smallest eigenvalue per row")
        for i in range(N_SECOND_LAP):
            print("%4d  %6.3f m  %6.3f m  %6d  %9d   %.4f" % (i, out["before"][i], out["after"][i], out["iterations"][i], out["rows"][i],
                                                             out["smallest_eigenvalue"][i]))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--leaf", type=float, default=0.5, help="voxel edge in metres")
    args = ap.parse_args()
    main(leaf=args.leaf)
