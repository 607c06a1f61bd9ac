#!/usr/bin/env python3
"""Map cleaning: the lot drive of examples/global_map.py with a car driving past, assembled into a cloud map and cleaned.

    python -m loam_amd.build            # once: libloamx.so + the pybind11 module
    python examples/clean_map.py [--leaf 0.3]

The scans are ray casts of the lot with a box of 4.4 x 1.8 x 1.6 m that moves 1.5 m from scan to scan. On the device, without the
data leaving it: the scans go into a cloud map at their poses (`add_clouds_dev`), the map's voxel centroids are emitted
(`emit_dev`), every centroid is voted on by every scan (`visibility_votes_dev`: did the beam towards it stop there, before it,
or pass through?), and the points that many scans saw through and few confirmed are taken out (`visibility_filter_dev`). The
program prints how many voxels of the moving box and how many of the rest of the map were removed.

The poses are the drive's true poses uploaded once; a vehicle hands over the trajectory buffer that `compose_trajectory_dev` or
`pose_graph_optimize_dev` left on the device, as examples/global_map.py does."""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import outdoor_scenes  # noqa: E402  (only for the stand-in scans)

_spec = importlib.util.spec_from_file_location("loop_closure_drive", os.path.join(os.path.dirname(os.path.abspath(__file__)), "loop_closure.py"))
loop_closure = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(loop_closure)

N_SCANS = loop_closure.N_SCANS
BOX = (4.4, 1.8, 1.6)
BOX_STEP = 1.5


def drive_scans(H, W):
    """(scans (n, H W, 3) float32, poses (n, 7), from_box (n, H W) bool: the return came from the moving box)"""
    poses = loop_closure.drive()
    boxes = outdoor_scenes.scene_boxes("lot", 0)
    o0 = poses[0][0]
    scans, from_box = [], []
    for i, (origin, yaw) in enumerate(poses):
        cx, cy = o0[0] - 7.5 + BOX_STEP * i, o0[1] + 6.5  # the car's lane, 6.5 m beside the circle the sensor drives
        car = outdoor_scenes._box(cx - BOX[0] / 2, cx + BOX[0] / 2, cy - BOX[1] / 2, cy + BOX[1] / 2, 0.0, BOX[2])
        fan = outdoor_scenes.FANS["lot"]
        with_car = outdoor_scenes.cast(boxes + [car], origin, yaw, H, W, fan, 0.01, np.random.default_rng(i))
        without = outdoor_scenes.cast(boxes, origin, yaw, H, W, fan, 0.01, np.random.default_rng(i))
        scans.append(with_car)
        from_box.append((with_car != without).any(axis=1))
    truth = np.array([outdoor_scenes.yaw_pose(yaw, origin) for origin, yaw in poses])
    return np.ascontiguousarray(scans, dtype=np.float32), np.ascontiguousarray(truth), np.array(from_box)


def voxel_keys(points, leaf):
    v = np.floor(points / leaf).astype(np.int64) + (1 << 20)
    return (v[:, 0] << 42) | (v[:, 1] << 21) | v[:, 2]


def box_share(scans, poses, from_box, centroids, leaf):
    """per centroid the share of its voxel's points that were returns from the moving box"""
    world, flags = [], []
    for scan, pose, fb in zip(scans, poses, from_box):
        yaw = 2.0 * np.arctan2(pose[2], pose[3])
        hit = np.any(scan != 0.0, axis=1)
        world.append(outdoor_scenes.to_world(scan[hit].astype(np.float64), pose[4:], yaw))
        flags.append(fb[hit])
    keys, flags = voxel_keys(np.concatenate(world), leaf), np.concatenate(flags)
    uniq, inverse = np.unique(keys, return_inverse=True)
    n_all, n_box = np.bincount(inverse), np.bincount(inverse, weights=flags.astype(np.float64))
    at = np.minimum(np.searchsorted(uniq, voxel_keys(centroids, leaf)), len(uniq) - 1)
    found = uniq[at] == voxel_keys(centroids, leaf)
    return np.where(found, n_box[at] / n_all[at], 0.0)


def main(scan_lines=32, points_per_line=512, leaf=0.3, max_voxels=1 << 18, verbose=True, ctx=None):
    from loam_amd import capi
    c = ctx or capi.Context(0)
    H, W, n = scan_lines, points_per_line, N_SCANS
    scans, poses, from_box = drive_scans(H, W)
    top, bottom = outdoor_scenes.FANS["lot"]
    elevations = np.radians(bottom + (top - bottom) * np.arange(H) / (H - 1))  # the beams of outdoor_scenes.beam_directions
    layout = c.scan_layout(capi.LidarParams(H, W, 1.0, 120.0), capi.OrganizeParams(elevations=elevations))
    cloud_map = c.cloud_map(capi.CloudMapParams(leaf=leaf), max_voxels)
    params = capi.VisibilityParams()
    bufs = []

    def room(nbytes):
        bufs.append(c.alloc(nbytes))
        return bufs[-1]

    try:
        d_scans, d_poses = room(scans.nbytes).upload(scans), room(poses.nbytes).upload(poses)
        d_xyz, d_n = room(max_voxels * 24), room(4)
        cloud_map.add_clouds_dev(d_scans.ptr, 3, np.arange(n + 1) * (H * W), d_poses.ptr, f32=True)
        cloud_map.emit_dev(d_xyz.ptr, max_voxels, d_n.ptr)
        n_vox = int(d_n.download(np.uint32, 1)[0])  # (four bytes: the sizes of the buffers below)
        d_votes, d_dynamic, d_static, d_n_static = room(n_vox * 16), room(n_vox), room(n_vox * 24), room(4)
        c.visibility_votes_dev(layout, d_xyz.ptr, 3, n_vox, d_scans.ptr, n, d_poses.ptr, d_votes.ptr, params, f32=True)
        c.visibility_filter_dev(d_votes.ptr, n_vox, d_n_static.ptr, params, d_xyz.ptr, 3, d_dynamic.ptr, d_static.ptr, 0, n_vox)
        n_static = int(d_n_static.download(np.uint32, 1)[0])
        out = dict(points=d_xyz.download(np.float64, 3 * n_vox).reshape(-1, 3), votes=d_votes.download(np.uint32, 4 * n_vox).view(capi.VISIBILITY_VOTES_DTYPE),
                   dynamic=d_dynamic.download(np.uint8, n_vox).astype(bool), static=d_static.download(np.float64, 3 * n_static).reshape(-1, 3),
                   census=c.last_visibility_census(), scans=scans, poses=poses, leaf=leaf, elevations=elevations)
    finally:
        cloud_map.close(), layout.close()
        for b in bufs:
            b.free()

    share = box_share(scans, poses, from_box, out["points"], leaf)
    out["is_box"], out["is_rest"] = share == 1.0, share == 0.0
    if verbose:
        box, rest, dyn = out["is_box"], out["is_rest"], out["dynamic"]
        print("%d scans of %d x %d points, leaf %.2f m: %d voxels, %d removed" % (n, H, W, leaf, len(dyn), int(dyn.sum())))
        print("  voxels of the moving box: %5d of %5d removed" % (int((dyn & box).sum()), int(box.sum())))
        print("  voxels of the rest:       %5d of %5d removed" % (int((dyn & rest).sum()), int(rest.sum())))
        print("  %d of %d (point, scan) pairs were in range, %d had a cell" % (out["census"].in_range_pairs, len(dyn) * n, out["census"].projected_pairs))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--leaf", type=float, default=0.3, help="voxel edge in metres")
    args = ap.parse_args()
    main(leaf=args.leaf)
