#!/usr/bin/env python3
"""Scan-to-map along a drive through the ray-cast street canyon of tests/outdoor_scenes.py.

    python -m loam_amd.build            # once: libloamx.so + the pybind11 module
    python examples/scan_to_map.py [n_scans]

1. Odometry: `loam.registerScanSequence` registers the consecutive scans of the drive (previous_T_current per pair).
2. Mapping, scan by scan: the chained odometry pose is the initial estimate of `loam.registerFeatures(features, map, init)`
   against the map held in a `loam.TargetIndex`; the refined pose moves the scan's features into the map frame,
   `insertFiltered` adds those whose voxel (0.2 m for edges, 0.4 m for planar points) is still empty, and `crop` drops what
   has left a window of +-40 m around the vehicle. Transform, voxel filter, insert and crop run on the device; the map
   never visits the host.

`TargetIndex`, the `registerFeatures` overload that takes it and `registerScanSequence` are extensions: the reference's
module has none of them. Without the filter the map grows by every scan's ~17 000 features; with it, by the few thousand
that show something new."""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "loam_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import loam  # noqa: E402
import outdoor_scenes as S  # noqa: E402

H, W, STEP = 64, 1024, 0.8
N_SCANS = int(sys.argv[1]) if len(sys.argv) > 1 else 12
EDGE_LEAF, PLANAR_LEAF, WINDOW = 0.2, 0.4, 40.0
lidar_params = loam.LidarParams(H, W, 1.0, 120.0)


def station(i):
    """(position, heading) of the sensor at scan i"""
    o0, yaw0 = S.sensor_origin("canyon", 3)
    return o0 + STEP * i * np.array([np.cos(yaw0), np.sin(yaw0), 0.0]), yaw0 + 0.006 * i


def true_pose(i):
    """ground truth scan0_T_scan_i as a loam.Pose3d"""
    a, b = S.yaw_pose(station(0)[1], station(0)[0]), S.yaw_pose(station(i)[1], station(i)[0])
    pa = loam.Pose3d(loam.Quaterniond(a[3], a[0], a[1], a[2]), a[4:])
    pb = loam.Pose3d(loam.Quaterniond(b[3], b[0], b[1], b[2]), b[4:])
    return pa.inverse().compose(pb)


scans = np.stack([S.scan_at("canyon", 0, *station(i), H, W, 0.01, noise_seed=1000 + i) for i in range(N_SCANS)])
steps = loam.registerScanSequence(scans, lidar_params)  # 1. odometry

features = [loam.extractFeatures(s, lidar_params) for s in scans]
local_map = loam.TargetIndex(features[0])  # the map frame is scan 0's
unfiltered = features[0].edge_points.shape[0] + features[0].planar_points.shape[0]
map_T_prev = loam.Pose3d.Identity()
print("scan  0: map %6d edge + %6d planar points" % (local_map.numEdgePoints(), local_map.numPlanarPoints()))
for i in range(1, N_SCANS):
    init = map_T_prev.compose(steps[i - 1])  # 2. the chained odometry pose as the initial estimate
    map_T_scan = loam.registerFeatures(features[i], local_map, init)
    added = local_map.insertFiltered(features[i], map_T_scan, edge_leaf=EDGE_LEAF, planar_leaf=PLANAR_LEAF)
    centre = np.asarray(map_T_scan.translation)
    removed = local_map.crop(centre - WINDOW, centre + WINDOW)
    unfiltered += features[i].edge_points.shape[0] + features[i].planar_points.shape[0]
    err = np.linalg.norm(np.asarray(true_pose(i).inverse().compose(map_T_scan).translation))
    print("scan %2d: + %4d / %5d of %4d / %5d features, - %4d / %5d outside the window -> map %6d edge + %6d planar points "
          "(unfiltered, uncropped: %7d); position error %.3f m" %
          (i, added[0], added[1], features[i].edge_points.shape[0], features[i].planar_points.shape[0], removed[0], removed[1],
           local_map.numEdgePoints(), local_map.numPlanarPoints(), unfiltered, err))
    map_T_prev = map_T_scan
