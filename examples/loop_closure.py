#!/usr/bin/env python3
"""Noticing that one has been here before: place recognition in front of the registration that makes a loop edge.

    python -m loam_amd.build            # once: libloamx.so + the pybind11 module
    python examples/loop_closure.py [--threshold 0.25] [--min-age 5]

A drive around the lot scene of tests/outdoor_scenes.py comes back to where it began, facing another way. Every scan's
descriptor (`loam.PlaceDatabase.descriptor`: a polar grid of maximum heights, computed on the device) goes into the database,
and every scan asks for the stored scans more than `min_age` scans old that look like it. A match under the threshold carries
the number of sectors the sensor is turned relative to the old scan: `PlaceMatch.initialGuess()` is that yaw as a pose, and
`registerFeatures` started from it gives old_T_new — the loop edge of a pose graph, whose information matrix
`loam.registrationInformation` would add. Without the yaw the registration would start a quarter turn or more from the truth,
far outside its basin."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (os.path.join(ROOT, "loam_amd", "python"), os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)
import outdoor_scenes  # noqa: E402  (only for the stand-in scans)

N_SCANS = 12
MIN_AGE = 5
THRESHOLD = 0.25


def drive(n=N_SCANS):
    """[(position, heading)]: once around a 3.5 m circle in the lot, heading along the tangent; the last pose is the first one's
    place again, 0.3 m off and turned by 100 degrees"""
    o0, yaw0 = outdoor_scenes.sensor_origin("lot", 0)
    centre = o0 - 3.5 * np.array([np.cos(yaw0 + np.pi / 2), np.sin(yaw0 + np.pi / 2), 0.0])
    poses = []
    for i in range(n - 1):
        a = 2.0 * np.pi * i / (n - 1)
        r = 3.5 * np.array([np.cos(yaw0 + np.pi / 2 + a), np.sin(yaw0 + np.pi / 2 + a), 0.0])
        poses.append((centre + r, yaw0 + a))
    poses.append((o0 + outdoor_scenes._rz(yaw0) @ np.array([0.25, 0.15, 0.0]), yaw0 + np.radians(100.0)))
    return poses


def relative_pose(old, new):
    """old_T_new of two (position, heading) poses as a pose7"""
    (o_old, yaw_old), (o_new, yaw_new) = old, new
    return outdoor_scenes.yaw_pose(yaw_new - yaw_old, outdoor_scenes._rz(-yaw_old) @ (o_new - o_old))


def pose7(pose):
    q, t = pose.rotation, pose.translation
    return np.array([q.x(), q.y(), q.z(), q.w(), t[0], t[1], t[2]])


def pose_errors(got, want):
    """(rotation angle, translation distance) between two pose7"""
    dq = abs(float(np.dot(got[:4], want[:4])))
    return 2.0 * np.arccos(min(1.0, dq)), float(np.linalg.norm(got[4:] - want[4:]))


def main(scan_lines=32, points_per_line=512, threshold=THRESHOLD, min_age=MIN_AGE, verbose=True):
    import loam
    lidar_params = loam.LidarParams(scan_lines, points_per_line, 1.0, 120.0)
    db = loam.PlaceDatabase()  # 20 rings x 60 sectors out to 80 m
    poses = drive()
    features, loops = [], []
    for i, (origin, yaw) in enumerate(poses):
        scan = np.ascontiguousarray(outdoor_scenes.scan_at("lot", 0, origin, yaw, scan_lines, points_per_line, noise_seed=i), dtype=np.float32)
        features.append(loam.extractFeatures(scan, lidar_params))
        desc = db.descriptor(scan)
        eligible = max(0, i - min_age + 1)  # the scans at least min_age old
        best = db.search(desc, 1, id_end=eligible)[0] if eligible else None
        assert db.add(desc) == i
        if best is None or not best.valid or best.distance >= threshold:
            if verbose:
                print("scan %2d: no place under %.2f%s" % (i, threshold, "" if best is None or not best.valid
                                                          else " (nearest: scan %d at %.3f)" % (best.id, best.distance)))
            continue
        old_T_new = pose7(loam.registerFeatures(source=features[i], target=features[best.id], target_T_source_init=best.initialGuess()))
        truth = relative_pose(poses[best.id], poses[i])
        rot_err, trans_err = pose_errors(old_T_new, truth)
        loops.append(dict(query=i, entry=int(best.id), distance=best.distance, shift=int(best.shift), pose=old_T_new, truth=truth,
                          rotation_error=rot_err, translation_error=trans_err))
        if verbose:
            print("scan %2d: the place of scan %d (distance %.3f), turned by %d sectors = %.0f degrees" % (i, best.id, best.distance, best.shift, np.degrees(best.yaw)))
            print("         registered: yaw %7.2f deg  t = %s" % (np.degrees(2 * np.arctan2(old_T_new[2], old_T_new[3])), np.round(old_T_new[4:], 3)))
            print("         truth:      yaw %7.2f deg  t = %s   (off by %.3f deg, %.3f m)"
                  % (np.degrees(2 * np.arctan2(truth[2], truth[3])), np.round(truth[4:], 3), np.degrees(rot_err), trans_err))
    return loops


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--threshold", type=float, default=THRESHOLD, help="a match counts as a loop under this descriptor distance")
    ap.add_argument("--min-age", type=int, default=MIN_AGE, help="only scans at least this many scans old are candidates")
    args = ap.parse_args()
    main(threshold=args.threshold, min_age=args.min_age)
