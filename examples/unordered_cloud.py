#!/usr/bin/env python3
"""From an unordered cloud to a pose: what a user with a real sensor does in front of the reference README's loop.

    python -m loam_amd.build            # once: libloamx.so + the pybind11 module
    python examples/unordered_cloud.py

A KITTI .bin is about 120 k unordered `x y z intensity` floats without a ring channel; every entry point of this library (and
of the reference) wants scan_lines x points_per_line points in row-major [line][column] order. `loam.organizeCloud` puts the
cloud into that grid on the device: the line of a point from its elevation (or from a ring number, where the driver gives
one), its column from its azimuth, one deterministic winner per cell, (0, 0, 0) where no point landed — which the extraction
takes for a beam without a return. The index map it returns gathers whatever else came with the points.

The clouds here are two canyon scans of tests/outdoor_scenes.py turned into what a file would hold: beams without a return
removed, the rest shuffled, float32 `x y z i`."""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (os.path.join(ROOT, "loam_amd", "python"), os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)
import loam  # noqa: E402
import outdoor_scenes  # noqa: E402  (only for the stand-in scans)


def as_file_cloud(scan, rng):
    """an organised scan -> (n, 4) float32 `x y z i` in no particular order, without the beams that returned nothing"""
    pts = scan[(scan != 0).any(axis=1)]
    pts = pts[rng.permutation(len(pts))]
    intensity = 1.0 / (1.0 + np.linalg.norm(pts, axis=1))  # (anything: it is not looked at)
    return np.ascontiguousarray(np.concatenate([pts, intensity[:, None]], axis=1), dtype=np.float32)


def pose7(pose):
    q, t = pose.rotation, pose.translation
    return np.array([q.x(), q.y(), q.z(), q.w(), t[0], t[1], t[2]])


def main(scan_lines=64, points_per_line=1024, verbose=True):
    lidar_params = loam.LidarParams(scan_lines, points_per_line, 1.0, 120.0)
    params = loam.OrganizeParams()
    top, bottom = outdoor_scenes.FANS["canyon"]  # the sensor's data sheet: the beams' elevations, lowest first
    params.elevations = list(np.radians(bottom + (top - bottom) * np.arange(scan_lines) / (scan_lines - 1)))
    layout = loam.ScanLayout(lidar_params, params)

    target_scan, source_scan, truth = outdoor_scenes.pair("canyon", 0, scan_lines, points_per_line)
    rng = np.random.default_rng(0)
    clouds = [as_file_cloud(s, rng) for s in (target_scan, source_scan)]  # stand-in for two files of a dataset

    world_T_lidar = loam.Pose3d.Identity()
    feat_prev = None
    for cloud in clouds:
        scan, src_idx = loam.organizeCloud(cloud, layout)          # (H W, 3) float32, and where every cell came from
        intensity = np.where(src_idx != 0xFFFFFFFF, cloud[np.minimum(src_idx, len(cloud) - 1), 3], 0.0)  # e.g. the fourth channel
        feat = loam.extractFeatures(scan, lidar_params)
        if feat_prev is not None:
            prev_T_cur = loam.registerFeatures(source=feat, target=feat_prev, target_T_source_init=loam.Pose3d.Identity())
            world_T_lidar = world_T_lidar.compose(prev_T_cur)
        feat_prev = feat
        if verbose:
            print("cloud of %d points -> %d of %d cells filled (mean intensity %.3f), %d edge / %d planar features"
                  % (len(cloud), int((src_idx != 0xFFFFFFFF).sum()), len(src_idx), float(intensity.mean()), len(feat.edge_points),
                     len(feat.planar_points)))
    pose = pose7(world_T_lidar)
    if verbose:
        # the same loop on the scans as they were before they became clouds: the organiser has put every point back in its cell,
        # so the features are the same points and the pose is the same bits
        feats = [loam.extractFeatures(np.ascontiguousarray(s, dtype=np.float32), lidar_params) for s in (target_scan, source_scan)]
        direct = pose7(loam.registerFeatures(source=feats[1], target=feats[0], target_T_source_init=loam.Pose3d.Identity()))
        print("pose from the clouds:          q = (%.6f %.6f %.6f %.6f)  t = %s" % (*pose[:4], np.round(pose[4:], 4)))
        print("pose from the organised scans: q = (%.6f %.6f %.6f %.6f)  t = %s  (%s)"
              % (*direct[:4], np.round(direct[4:], 4), "identical" if np.array_equal(pose, direct) else "DIFFERENT"))
        print("the scene's ground truth:      q = (%.6f %.6f %.6f %.6f)  t = %s  (a canyon constrains the motion along its axis "
              "weakly: see examples/degeneracy.py)" % (*truth[:4], np.round(truth[4:], 4)))
    return pose


if __name__ == "__main__":
    main()
