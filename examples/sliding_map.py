#!/usr/bin/env python3
"""A map of fixed size that follows the sensor: localise, add, crop, for a drive longer than the map's capacity.

    python -m loam_amd.build            # once: libloamx.so + the pybind11 module
    python examples/sliding_map.py [--scans 120] [--half 15] [--max-voxels 8192]

The drive runs down the street of the canyon scene of tests/outdoor_scenes.py, 0.8 m per scan. The first four scans go into a
surfel map at their poses. Every later scan starts from an odometry pose (the true pose off by 0.1 m and half a degree, fixed
seed), is placed on the map by the surfel localiser, is added at the pose the localiser wrote, and the map is cropped to a
window of +-`--half` metres around that pose. The pose never leaves the device: the add and the crop read it where the
localiser left it, and the whole drive is enqueued with ONE synchronise at its end. The program prints the voxel count of the map
after every crop and the overflow of the map (0), and beside it the overflow of a second map of the same max_voxels that takes the
same scans at the same poses and is never cropped."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)
import outdoor_scenes  # noqa: E402  (only for the stand-in scans)

N_SEED = 4  # scans that go into the map at their true poses before the loop begins


def drive(n_scans, step=0.8):
    """[(position, heading)] down the street, from its western end"""
    return [(np.array([-50.0 + step * i, 0.4 * np.sin(0.05 * i), outdoor_scenes.SENSOR_HEIGHT]), 0.02 * np.sin(0.03 * i)) for i in range(n_scans)]


def odometry(origin, yaw, seed, metres=0.1, degrees=0.5):
    """the true pose off by that much, as pose7"""
    rng = np.random.default_rng([23, seed])
    t = rng.normal(size=3) * [1.0, 1.0, 0.2]
    return outdoor_scenes.yaw_pose(yaw + np.radians(degrees) * rng.choice([-1.0, 1.0]), origin + t / np.linalg.norm(t) * metres)


def main(scan_lines=16, points_per_line=256, n_scans=120, leaf=0.5, half=15.0, max_voxels=8192, verbose=True):
    from loam_amd import capi
    H, W = scan_lines, points_per_line
    per = H * W
    path = drive(n_scans)
    scans = np.ascontiguousarray([outdoor_scenes.scan_at("canyon", 0, o, yaw, H, W, noise_seed=i) for i, (o, yaw) in enumerate(path)], dtype=np.float32)
    true = np.ascontiguousarray([outdoor_scenes.yaw_pose(yaw, o) for o, yaw in path])
    start = np.ascontiguousarray([odometry(o, yaw, i) for i, (o, yaw) in enumerate(path)])

    ctx = capi.Context(0)
    params = capi.SurfelMapParams(leaf=leaf)
    sliding, uncropped = ctx.surfel_map(params, max_voxels), ctx.surfel_map(params, max_voxels)
    loc = sliding.localizer(1, per)
    d_scans, d_true, d_start = ctx.alloc(scans.nbytes).upload(scans), ctx.alloc(true.nbytes).upload(true), ctx.alloc(start.nbytes).upload(start)
    d_poses, d_results, d_counts = ctx.alloc(n_scans * 56), ctx.alloc(n_scans * 128), ctx.alloc(n_scans * 16)
    lo, hi = [-half, -half, -np.inf], [half, half, np.inf]
    try:
        seed_offsets = np.arange(N_SEED + 1) * per
        sliding.add_clouds_dev(d_scans.ptr, 3, seed_offsets, d_true.ptr, f32=True)
        uncropped.add_clouds_dev(d_scans.ptr, 3, seed_offsets, d_true.ptr, f32=True)
        for i in range(N_SEED, n_scans):
            scan, pose = d_scans.ptr + i * per * 12, d_poses.ptr + i * 56
            loc.run_dev(scan, 3, [0, per], d_start.ptr + i * 56, pose, d_results.ptr + i * 128, f32=True)
            sliding.add_clouds_dev(scan, 3, [0, per], pose, f32=True)
            sliding.crop_dev(lo, hi, pose, d_counts.ptr + i * 16)
            uncropped.add_clouds_dev(scan, 3, [0, per], pose, f32=True)
        ctx.synchronize()  # the only one: nothing above waited for the device
        poses = d_poses.download(np.float64, n_scans * 7).reshape(n_scans, 7)[N_SEED:]
        results = d_results.download(capi.LOCALIZE_RESULT_DTYPE, n_scans)[N_SEED:]
        counts = d_counts.download(np.uint32, n_scans * 4).reshape(n_scans, 4)[N_SEED:]
        st, st_uncropped = sliding.stats(), uncropped.stats()
    finally:
        loc.close(), sliding.close(), uncropped.close()
        for b in (d_scans, d_true, d_start, d_poses, d_results, d_counts):
            b.free()
        ctx.close()
    out = dict(max_voxels=max_voxels, voxels=counts[:, 0].astype(int).tolist(), removed=counts[:, 1].astype(int).tolist(),
               skipped=int(counts[:, 2].sum()), overflow=int(st["overflow"]), final_voxels=int(st["voxels"]),
               uncropped_overflow=int(st_uncropped["overflow"]), uncropped_voxels=int(st_uncropped["voxels"]),
               error=np.linalg.norm(poses[:, 4:] - true[N_SEED:, 4:], axis=1).tolist(), termination=results["termination"].astype(int).tolist(),
               poses=poses, true_poses=true[N_SEED:])
    if verbose:
        print("a drive of %d scans of %d x %d points, %.0f m; leaf %.2f m, max_voxels %d, window +-%.0f m"
              % (n_scans, H, W, 0.8 * (n_scans - 1), leaf, max_voxels, half))
        print("scan   voxels after the crop   removed   distance to the true pose")
        for k in range(len(counts)):
            print("%4d  %10d  %16d   %8.3f m" % (N_SEED + k, counts[k, 0], counts[k, 1], out["error"][k]))
        print("the cropped map: overflow == %d, %d voxels at the end (most before a crop: %d)"
              % (out["overflow"], out["final_voxels"], int((counts[:, 0] + counts[:, 1]).max())))
        print("the same scans at the same poses without a crop: %d voxels listed, overflow == %d" % (out["uncropped_voxels"], out["uncropped_overflow"]))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scans", type=int, default=120)
    ap.add_argument("--half", type=float, default=15.0, help="half the window's edge in metres")
    ap.add_argument("--max-voxels", type=int, default=8192)
    args = ap.parse_args()
    main(n_scans=args.scans, half=args.half, max_voxels=args.max_voxels)
