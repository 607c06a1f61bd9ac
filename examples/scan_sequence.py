#!/usr/bin/env python3
"""A drive through the ray-cast street canyon of tests/outdoor_scenes.py, registered as ONE scan sequence.

    python -m loam_amd.build            # once: libloamx.so + the pybind11 module
    python examples/scan_sequence.py

1. `loam.registerScanSequence` takes the consecutive scans of the drive and returns previous_T_current of every consecutive
   pair; every scan is uploaded and extracted once (the reference's loop, examples/scan_to_scan.py, as one call).
2. The chained trajectory is composed on the device from the result records (`Context.compose_trajectory_dev`).
3. `loam.deskewScan` removes the motion of a sweep from a scan. The ray caster takes a scan from one pose, so a moving
   sweep is assembled from 16 casts at poses along the motion, 64 columns from each; registered against the previous scan
   as it is, its rotation comes out ~0.2 degrees off; after the correction (motion = the drive's previous step, constant
   velocity) ~0.01 degrees, like the scans taken standing still.

`registerScanSequence` and `deskewScan` are extensions: the reference's module has neither.

On this scene every step comes out ~0.1 m short of the true 0.8 m. That is the algorithm on a flat ray-cast ground, whose
rings travel with the sensor, not this implementation: the CPU oracle returns the same poses to 1e-15
(tests/test_gpu_sequence.py). The rotation shows what the motion correction is worth."""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "loam_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import loam  # noqa: E402
import outdoor_scenes as S  # noqa: E402
from loam_amd import capi  # noqa: E402

H, W, N_SCANS, STEP = 64, 1024, 6, 0.8
lidar_params = loam.LidarParams(H, W, 1.0, 120.0)


def station(i):
    """(position, heading) of the sensor at time i (in scans; fractions lie between two scans)"""
    o0, yaw0 = S.sensor_origin("canyon", 3)
    return o0 + STEP * i * np.array([np.cos(yaw0), np.sin(yaw0), 0.0]), yaw0 + 0.006 * i


def pose_of(p):
    r = p.rotation
    return np.array([r.x(), r.y(), r.z(), r.w(), *p.translation])


def relative(i, j):
    """ground truth i_T_j of two stations as a loam.Pose3d"""
    (oi, yi), (oj, yj) = station(i), station(j)
    a = S.yaw_pose(yi, oi)
    b = S.yaw_pose(yj, oj)
    pa = loam.Pose3d(loam.Quaterniond(a[3], a[0], a[1], a[2]), a[4:])
    pb = loam.Pose3d(loam.Quaterniond(b[3], b[0], b[1], b[2]), b[4:])
    return pa.inverse().compose(pb)


def error(est, truth):
    d = pose_of(truth.inverse().compose(est))
    return 2 * np.degrees(np.arctan2(np.linalg.norm(d[:3]), abs(d[3]))), np.linalg.norm(d[4:])


scans = np.stack([S.scan_at("canyon", 0, *station(i), H, W, 0.01, noise_seed=1000 + i) for i in range(N_SCANS)])

# 1. the sequence in one call
steps = loam.registerScanSequence(scans, lidar_params)
for i, prev_T_cur in enumerate(steps):
    rot, trans = error(prev_T_cur, relative(i, i + 1))
    print("pair %d: t = %s   error vs ground truth %.4f deg %.4f m" % (i, np.round(prev_T_cur.translation, 4), rot, trans))

# 2. the trajectory, composed on the device from the records of the device-resident form
ctx = capi.Context(0)
lidar = capi.LidarParams(H, W, 1.0, 120.0)
d_xyz, d_res, d_traj = ctx.alloc(scans.nbytes).upload(scans), ctx.alloc((N_SCANS - 1) * 64), ctx.alloc(N_SCANS * 56)
ctx.register_scan_sequence_dev(d_xyz.ptr, N_SCANS, lidar, capi.FeatureExtractionParams(), capi.RegistrationParams(), d_res.ptr)
origin = S.yaw_pose(station(0)[1], station(0)[0])
ctx.compose_trajectory_dev(d_res.ptr, N_SCANS - 1, d_traj.ptr, origin)
ctx.synchronize()
traj = d_traj.download(np.float64, N_SCANS * 7).reshape(N_SCANS, 7)
for i in range(N_SCANS):
    print("world_T_scan[%d]: t = %s   true position %s" % (i, np.round(traj[i, 4:], 3), np.round(station(i)[0], 3)))
for b in (d_xyz, d_res, d_traj):
    b.free()

# 3. a sweep taken while the sensor moves from station 3 to station 4, with and without motion correction
K = 16
moving = np.empty((H, W, 3))
for k in range(K):
    cols = slice(k * W // K, (k + 1) * W // K)
    part = S.scan_at("canyon", 0, *station(3 + (k + 0.5) / K), H, W, 0.01, noise_seed=2000 + k).reshape(H, W, 3)
    moving[:, cols] = part[:, cols]
moving = np.ascontiguousarray(moving.reshape(-1, 3))
truth = relative(2, 3)  # scan 2 -> the START of the sweep
raw = loam.registerScanSequence(np.stack([scans[2], moving]), lidar_params)[0]
corrected_scan = loam.deskewScan(moving, lidar_params, motion=steps[2], ref_fraction=0.0)  # constant velocity: the previous step
fixed = loam.registerScanSequence(np.stack([scans[2], corrected_scan]), lidar_params)[0]
print("moving sweep as it is:      error %.4f deg %.4f m" % error(raw, truth))
print("moving sweep, de-skewed:    error %.4f deg %.4f m" % error(fixed, truth))
