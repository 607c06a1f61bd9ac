#!/usr/bin/env python3
"""Measurements of the cloud map; writes profiles/cloudmap_bench.json. Run on a GPU box.

    python tools/bench_cloudmap.py [--scans 256] [--leaf 0.2] [--out profiles/cloudmap_bench.json]

1. add: `--scans` resident 64 x 1024 scans of the canyon drive of tools/bench_map.py at their ground-truth poses (device
   poses), one loamx_cloud_map_add_clouds_dev_f32 call into a cleared map, with run combining and without
   (NO_CLOUDMAP_COMBINE), alternating in one process on the same inputs, median of 9 calls after 2; both forms must leave
   the same stats and the same emitted bytes.
2. emit: loamx_cloud_map_emit_dev of the assembled map, median of 9 after 2.
3. atomics per point: a claim costs one CAS (more when the probe walks) and five atomics; the kernel counts its claims
   (loamx_cloud_map_claims_read): once per used point in the plain form, once per run of a wavefront with combining."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cloudmap_common as M  # noqa: E402
import outdoor_scenes as S  # noqa: E402
from loam_amd import build as B  # noqa: E402
from loam_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scans", type=int, default=256)
ap.add_argument("--leaf", type=float, default=0.2)
ap.add_argument("--max-voxels", type=int, default=1 << 22)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloudmap_bench.json"))
args = ap.parse_args()
ctx = capi.Context(0)
H, W, n = 64, 1024, args.scans
params = capi.CloudMapParams(leaf=args.leaf)

o0, yaw0 = S.sensor_origin("canyon", 3)
scans, poses = [], []
for i in range(n):
    origin, yaw = o0 + 0.8 * i * np.array([np.cos(yaw0), np.sin(yaw0), 0.0]), yaw0 + 0.006 * i
    scans.append(S.scan_at("canyon", 0, origin, yaw, H, W, 0.01, noise_seed=1000 + i).astype(np.float32))
    poses.append(S.yaw_pose(yaw, origin))
scans, poses = np.ascontiguousarray(scans), np.ascontiguousarray(poses)
offsets = np.arange(n + 1) * (H * W)
d_scans, d_poses = ctx.alloc(scans.nbytes).upload(scans), ctx.alloc(poses.nbytes).upload(poses)
d_xyz, d_n = ctx.alloc(args.max_voxels * 24), ctx.alloc(4)
cmap = ctx.cloud_map(params, args.max_voxels)


def add(plain):
    ctx.set_option("NO_CLOUDMAP_COMBINE", plain)
    cmap.clear()
    ctx.synchronize()
    t0 = time.perf_counter()
    cmap.add_clouds_dev(d_scans.ptr, 3, offsets, d_poses.ptr, f32=True)
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def emit():
    ctx.synchronize()
    t0 = time.perf_counter()
    cmap.emit_dev(d_xyz.ptr, args.max_voxels, d_n.ptr)
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


times, seen, claims = {0: [], 1: []}, {}, {}
for rep in range(11):
    for plain in (0, 1):
        times[plain].append(add(plain))
        if rep == 0:
            emit()
            k = int(d_n.download(np.uint32, 1)[0])
            seen[plain] = ({name: int(cmap.stats()[name]) for name in M.STAT_NAMES}, d_xyz.download(np.float64, 3 * min(k, args.max_voxels)).tobytes())
            claims[plain] = cmap.claims()
assert seen[0] == seen[1], "run combining changed the map"
stats = seen[0][0]
t_emit = [emit() for _ in range(11)]
ctx.set_option("NO_CLOUDMAP_COMBINE", 0)

med = {k: statistics.median(v[2:]) for k, v in times.items()}
points = n * H * W
out = dict(source_hash=B.source_hash(), scans=n, scan_shape=[H, W], points=points, leaf=args.leaf, max_voxels=args.max_voxels, stats=stats,
           add_ms_median=dict(combined=round(med[0], 3), plain=round(med[1], 3)),
           add_ms=dict(combined=[round(t, 3) for t in times[0][2:]], plain=[round(t, 3) for t in times[1][2:]]),
           add_points_per_s=dict(combined=round(points / med[0] * 1e3), plain=round(points / med[1] * 1e3)),
           emit_ms_median=round(statistics.median(t_emit[2:]), 3), emit_ms=[round(t, 3) for t in t_emit[2:]], emit_voxels=stats["voxels"],
           claims=dict(combined=claims[0], plain=claims[1]),
           claims_per_offered_point=dict(combined=round(claims[0] / max(points, 1), 4), plain=round(claims[1] / max(points, 1), 4)),
           points_per_claim=dict(combined=round(stats["points_used"] / max(claims[0], 1), 3), plain=round(stats["points_used"] / max(claims[1], 1), 3)),
           atomics_per_offered_point=dict(combined=round(6 * claims[0] / max(points, 1), 3), plain=round(6 * claims[1] / max(points, 1), 3)))
assert claims[1] == stats["points_used"], "the plain form claims once per used point"
print(json.dumps(out), flush=True)
cmap.close()
for b in (d_scans, d_poses, d_xyz, d_n):
    b.free()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
