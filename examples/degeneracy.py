#!/usr/bin/env python3
"""A drive out of the end of a hall into a long corridor: the smallest eigenvalue of the registration information matrix
falls where the geometry stops constraining the motion, and its eigenvector names the direction.

    python -m loam_amd.build            # once: libloamx.so + the pybind11 module
    python examples/degeneracy.py

The scene is a box 4 m wide and 3 m high whose end walls stand at y = 0 and y = 400; the sensor sees 12 m. It starts 4 m
from the near end wall and drives 1 m per scan along the axis. While the end wall is in range, its points hold the
translation along the corridor and the registration finds the step; once it is out of range only the side walls, the floor
and the ceiling are left, their residuals are blind to a shift along y, and the registration returns a step of zero with
CONVERGED — the pose alone does not say that anything went wrong. `Context.register_scan_sequence_dev(..., d_info=...)`
returns, next to every pose, the 6x6 information matrix of the residuals at that pose with its eigenpairs (include/loamx.h:
loamx_reg_information; basis: rotation vector about the target frame's axes, then translation in metres). Its smallest
eigenvalue belongs to t_y throughout and falls from ~340 (wall 5 m behind) to ~100 once the wall is gone. It does not reach
zero on this scene: where the five nearest target features of a wall point lie in one vertical column of the scan pattern
they are collinear, and the plane fitted through them may face along the corridor (the reference's fit has no test for
that). `degenerate_directions(threshold)` is what a mapper thresholds, and `covariance()` is what a pose graph or a filter
takes next to the pose."""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from loam_amd import capi  # noqa: E402

H, W, MAX_RANGE, STEP, N_SCANS, THRESHOLD = 64, 256, 12.0, 1.0, 14, 130.0
LO, HI = np.array([-2.0, 0.0, -1.5]), np.array([2.0, 400.0, 1.5])


def scan_at(y, seed):
    """H x W beams from (0.1, y, -0.2) against the inside of the box; 2 mm of range noise"""
    origin = np.array([0.1, y, -0.2])
    az = (np.arange(W) + 0.5) / W * 2 * np.pi
    el = np.radians(np.linspace(-40.0, 40.0, H))
    d = np.stack([np.cos(el)[:, None] * np.cos(az)[None, :], np.cos(el)[:, None] * np.sin(az)[None, :],
                  np.sin(el)[:, None] * np.ones(W)[None, :]], -1).reshape(-1, 3)
    with np.errstate(divide="ignore"):
        t = np.where(d > 0, (HI - origin) / d, (LO - origin) / d)  # distance to the wall each axis runs into
    r = t.min(axis=1) + np.random.default_rng(seed).normal(0.0, 0.002, len(d))
    return d * r[:, None]  # in the sensor frame (axes parallel to the world's)


ys = 4.0 + STEP * np.arange(N_SCANS)
scans = np.ascontiguousarray(np.stack([scan_at(y, 100 + i) for i, y in enumerate(ys)]))
ctx = capi.Context(0)
lidar, fe, reg = capi.LidarParams(H, W, 1.0, MAX_RANGE), capi.FeatureExtractionParams(), capi.RegistrationParams()
n_pairs = N_SCANS - 1
d_xyz, d_res, d_info = ctx.alloc(scans.nbytes).upload(scans), ctx.alloc(n_pairs * 64), ctx.alloc(n_pairs * capi.INFORMATION_DTYPE.itemsize)
ctx.register_scan_sequence_dev(d_xyz.ptr, N_SCANS, lidar, fe, reg, d_res.ptr, d_info=d_info.ptr)
ctx.synchronize()
results, records = d_res.download(capi.RESULT_DTYPE, n_pairs), d_info.download(capi.INFORMATION_DTYPE, n_pairs)
names = ["rx", "ry", "rz", "tx", "ty", "tz"]
print("scan  y [m]  end wall  rows   smallest eigenvalue   unconstrained        estimated step   sigma(ty) [m]")
for p in range(n_pairs):
    info = capi.RegInformation.from_record(records[p])
    y = ys[p + 1]
    loose = ["%s%+.2f" % (names[int(np.argmax(np.abs(v)))], v[int(np.argmax(np.abs(v)))]) for v in info.degenerate_directions(THRESHOLD)]
    rows = int(info.n_edge) + int(info.n_plane)
    sigma = "%.4f" % np.sqrt(info.covariance()[4, 4]) if rows > 6 and not loose else "unobservable"
    print("%4d  %5.1f  %-8s  %5d  %18.3f   %-18s  %14.3f   %s" % (
        p + 1, y, "in range" if y < MAX_RANGE else "gone", rows, info.eigenvalues[0], ", ".join(loose) or "-", results[p]["pose"][5], sigma))
for b in (d_xyz, d_res, d_info):
    b.free()
