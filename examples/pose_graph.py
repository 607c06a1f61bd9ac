#!/usr/bin/env python3
"""Closing the loop: the drive of examples/loop_closure.py as a pose graph, corrected on the device.

    python -m loam_amd.build            # once: libloamx.so + the pybind11 module
    python examples/pose_graph.py [--huber 0]

The scans of the drive are registered as a sequence with information (`register_scan_sequence_dev`: pair p has scan p as its
target and scan p + 1 as its source, each result comes with its 6 x 6 information matrix), the trajectory is composed from the
results on the device (`compose_trajectory_dev`) and the results become the odometry edges of a pose graph without leaving the
device (`pose_graph_edges_from_results_dev`). The place database notices that the last scan stands where the first one stood;
the registration started from the match's yaw gives the loop edge old_T_new, `registration_information` its weight. One call
(`pose_graph_optimize_dev`) then corrects every pose of the trajectory in place. The program prints how far the last pose is from
the truth before and after.

The registrations of consecutive scans start from a motion prior, as a vehicle's wheel odometry would supply it: the true
motion, off by a degree or two and a decimetre (consecutive scans lie 2 m apart and differ in heading by 33 degrees, the last
pair by 130: too far for a start at the identity)."""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)
import outdoor_scenes  # noqa: E402  (only for the stand-in scans)

_spec = importlib.util.spec_from_file_location("loop_closure_drive", os.path.join(os.path.dirname(os.path.abspath(__file__)), "loop_closure.py"))
loop_closure = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(loop_closure)

N_SCANS = loop_closure.N_SCANS
MIN_AGE = loop_closure.MIN_AGE
THRESHOLD = loop_closure.THRESHOLD


def world_pose(pose):
    """world_T_sensor of a (position, heading) pose as a pose7"""
    origin, yaw = pose
    return outdoor_scenes.yaw_pose(yaw, origin)


def motion_priors(poses, seed=5, yaw_sigma=np.radians(1.5), trans_sigma=0.1):
    """p_T_(p + 1) of consecutive poses as an odometer would report it: the truth with noise"""
    rng = np.random.default_rng(seed)
    out = []
    for old, new in zip(poses[:-1], poses[1:]):
        (o_old, yaw_old), (o_new, yaw_new) = old, new
        t = outdoor_scenes._rz(-yaw_old) @ (o_new - o_old) + trans_sigma * rng.normal(size=3) * np.array([1.0, 1.0, 0.2])
        out.append(outdoor_scenes.yaw_pose(yaw_new - yaw_old + yaw_sigma * rng.normal(), t))
    return np.ascontiguousarray(out, dtype=np.float64)


def main(scan_lines=32, points_per_line=512, huber_delta=0.0, threshold=THRESHOLD, min_age=MIN_AGE, verbose=True, ctx=None, stage_hook=None):
    """stage_hook(stage, ctx, d_scans, d_traj): called with "odometry" once the composed trajectory stands in d_traj and with
    "corrected" right behind the solve, before anything synchronises (examples/global_map.py assembles its maps there)"""
    from loam_amd import capi
    c = ctx or capi.Context(0)
    H, W, n = scan_lines, points_per_line, N_SCANS
    lidar, fe, reg = capi.LidarParams(H, W, 1.0, 120.0), capi.FeatureExtractionParams(), capi.RegistrationParams()
    poses = loop_closure.drive()
    truth = np.array([world_pose(p) for p in poses])
    scans = np.ascontiguousarray([outdoor_scenes.scan_at("lot", 0, o, yaw, H, W, noise_seed=i) for i, (o, yaw) in enumerate(poses)], dtype=np.float32)
    priors = motion_priors(poses)

    bufs = []

    def room(nbytes):
        bufs.append(c.alloc(nbytes))
        return bufs[-1]

    db = c.place_db()
    try:
        # odometry: the sequence with information, the trajectory and the edges, all on the device
        d_xyz, d_init = room(scans.nbytes).upload(scans), room(priors.nbytes).upload(priors)
        d_results, d_info = room((n - 1) * capi.RESULT_DTYPE.itemsize), room((n - 1) * capi.INFORMATION_DTYPE.itemsize)
        d_traj, d_edges = room(n * 7 * 8), room(n * capi.PGO_EDGE_DTYPE.itemsize)
        d_summary = room(capi.PGO_SUMMARY_DTYPE.itemsize)
        c.register_scan_sequence_dev(d_xyz.ptr, n, lidar, fe, reg, d_results.ptr, d_init.ptr, f32=True, d_info=d_info.ptr)
        c.compose_trajectory_dev(d_results.ptr, n - 1, d_traj.ptr, origin=truth[0])
        c.pose_graph_edges_from_results_dev(d_results, d_info, n - 1, d_edges)
        c.synchronize()
        odometry = d_traj.download(np.float64, n * 7).reshape(n, 7)
        if stage_hook:
            stage_hook("odometry", c, d_xyz, d_traj)

        # the loop: the last scan against the stored scans at least min_age old
        descs = [db.descriptor(s) for s in scans]
        db.add(np.stack(descs[:n - min_age]))
        best = db.search(descs[-1], 1)[0, 0]
        if best["id"] == capi.PLACE_NO_ID or best["distance"] >= threshold:
            raise RuntimeError("the place database found no loop for the last scan")
        old, new = int(best["id"]), n - 1
        feats = {}
        for i in (old, new):
            e, p = c.extract_features(scans[i], lidar, fe)
            feats[i] = (scans[i][e].astype(np.float64), scans[i][p].astype(np.float64))
        guess = outdoor_scenes.yaw_pose(2.0 * np.pi * int(best["shift"]) / db.n_sectors, np.zeros(3))
        old_T_new, _, _ = c.register_features(feats[new][0], feats[new][1], feats[old][0], feats[old][1], guess, reg)
        info = c.registration_information(feats[new][0], feats[new][1], feats[old][0], feats[old][1], old_T_new, reg)
        loop = np.zeros(1, dtype=capi.PGO_EDGE_DTYPE)
        loop["a"], loop["b"], loop["a_T_b"], loop["information"] = old, new, old_T_new, np.asarray(info.information).reshape(6, 6)
        c._check(c.lib.loamx_copy_to_device(c.h, d_edges.ptr + (n - 1) * capi.PGO_EDGE_DTYPE.itemsize, loop.ctypes.data, loop.nbytes))

        # one call corrects the trajectory in place (pose 0 stays where it is)
        c.pose_graph_optimize_dev(d_traj, n, d_edges, n, params=capi.PgoParams(huber_delta=huber_delta), d_summary=d_summary)
        if stage_hook:
            stage_hook("corrected", c, d_xyz, d_traj)
        c.synchronize()
        corrected = d_traj.download(np.float64, n * 7).reshape(n, 7)
        edges = d_edges.download(capi.PGO_EDGE_DTYPE, n)
        summary = d_summary.download(capi.PGO_SUMMARY_DTYPE, 1)[0]
    finally:
        db.close()
        for b in bufs:
            b.free()

    before = float(np.linalg.norm(odometry[-1, 4:] - truth[-1, 4:]))
    after = float(np.linalg.norm(corrected[-1, 4:] - truth[-1, 4:]))
    err = lambda T: np.linalg.norm(T[:, 4:] - truth[:, 4:], axis=1)
    if verbose:
        print("loop edge: scan %d is the place of scan %d (descriptor distance %.3f, turned by %d sectors)" % (new, old, best["distance"], best["shift"]))
        print("solve: cost %.4g -> %.4g in %d iterations (%d accepted, %d PCG iterations), %s"
              % (summary["initial_cost"], summary["final_cost"], summary["iterations"], summary["accepted"], summary["pcg_iterations"],
                 capi.PGO_TERMINATIONS[summary["termination"]]))
        print("distance of every pose to the truth [m]")
        print("  odometry : " + " ".join("%.3f" % v for v in err(odometry)))
        print("  corrected: " + " ".join("%.3f" % v for v in err(corrected)))
        print("last pose: %.3f m from the truth before the optimisation, %.3f m after" % (before, after))
    return dict(loop=(old, new), before=before, after=after, odometry=odometry, corrected=corrected, truth=truth, edges=edges,
                termination=capi.PGO_TERMINATIONS[summary["termination"]], summary=summary)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--huber", type=float, default=0.0, help="huber_delta of the solve (0: off)")
    args = ap.parse_args()
    main(huber_delta=args.huber)
