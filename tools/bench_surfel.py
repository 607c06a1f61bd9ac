#!/usr/bin/env python3
"""Measurements of the surfel map; writes profiles/surfel_bench.json. Run on a GPU box.

    python tools/bench_surfel.py [--scans 256] [--leaf 0.5] [--out profiles/surfel_bench.json]

The workload of tools/bench_cloudmap.py: `--scans` resident 64 x 1024 float scans of the canyon drive at their ground-truth poses
(device poses).
1. add: one loamx_surfel_map_add_clouds_f32 call into a cleared map, with run combining and without (NO_SURFEL_COMBINE),
   alternating in one process on the same inputs, median of 9 calls after 2; both forms must leave the same stats and the same
   emitted bytes. The kernel counts its claims (loamx_surfel_map_claims_read): each is one CAS chain and fourteen atomics.
2. the yardstick: loamx_cloud_map_add_clouds_dev_f32 (with its run combining) on the same scans at the same leaf, in the same
   alternation.
3. emit: loamx_surfel_map_emit of the assembled map (records, means and normals), median of 9 after 2.
4. query: loamx_surfel_map_query of the emitted means (records, distances and counts), median of 9 after 2."""
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
import outdoor_scenes as S  # noqa: E402
from loam_amd import build as B  # noqa: E402
from loam_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scans", type=int, default=256)
ap.add_argument("--leaf", type=float, default=0.5)
ap.add_argument("--max-voxels", type=int, default=1 << 21)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surfel_bench.json"))
args = ap.parse_args()
ctx = capi.Context(0)
H, W, n = 64, 1024, args.scans
REC = capi.SURFEL_DTYPE.itemsize
STAT_NAMES = capi.SURFEL_MAP_STATS_DTYPE.names

o0, yaw0 = S.sensor_origin("canyon", 3)
scans, poses = [], []
for i in range(n):
    origin, yaw = o0 + 0.8 * i * np.array([np.cos(yaw0), np.sin(yaw0), 0.0]), yaw0 + 0.006 * i
    scans.append(S.scan_at("canyon", 0, origin, yaw, H, W, 0.01, noise_seed=1000 + i).astype(np.float32))
    poses.append(S.yaw_pose(yaw, origin))
scans, poses = np.ascontiguousarray(scans), np.ascontiguousarray(poses)
offsets = np.arange(n + 1) * (H * W)
d_scans, d_poses = ctx.alloc(scans.nbytes).upload(scans), ctx.alloc(poses.nbytes).upload(poses)
d_rec, d_xyz, d_normal, d_n = ctx.alloc(args.max_voxels * REC), ctx.alloc(args.max_voxels * 24), ctx.alloc(args.max_voxels * 24), ctx.alloc(4)
d_qrec, d_qdist, d_qcnt = ctx.alloc(args.max_voxels * REC), ctx.alloc(args.max_voxels * 8), ctx.alloc(args.max_voxels * 4)
smap = ctx.surfel_map(capi.SurfelMapParams(leaf=args.leaf), args.max_voxels)
cmap = ctx.cloud_map(capi.CloudMapParams(leaf=args.leaf), args.max_voxels)


def timed(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def add(plain):
    ctx.set_option("NO_SURFEL_COMBINE", plain)
    smap.clear()
    return timed(lambda: smap.add_clouds_dev(d_scans.ptr, 3, offsets, d_poses.ptr, f32=True))


def add_cloud_map():
    cmap.clear()
    return timed(lambda: cmap.add_clouds_dev(d_scans.ptr, 3, offsets, d_poses.ptr, f32=True))


def emit():
    return timed(lambda: smap.emit_dev(args.max_voxels, d_n.ptr, 1, d_rec.ptr, d_xyz.ptr, d_normal.ptr))


times, t_cloud, seen, claims = {0: [], 1: []}, [], {}, {}
for rep in range(11):
    for plain in (0, 1):
        times[plain].append(add(plain))
        if rep == 0:
            emit()
            k = int(d_n.download(np.uint32, 1)[0])
            seen[plain] = ({name: int(smap.stats()[name]) for name in STAT_NAMES}, d_rec.download(np.uint8, REC * min(k, args.max_voxels)).tobytes())
            claims[plain] = smap.claims()
    t_cloud.append(add_cloud_map())
assert seen[0] == seen[1], "run combining changed the map"
stats = seen[0][0]
assert stats["overflow"] == 0, "the map is too small for the drive: raise --max-voxels"
ctx.set_option("NO_SURFEL_COMBINE", 0)
add(0)
t_emit = [emit() for _ in range(11)]
k = int(d_n.download(np.uint32, 1)[0])
t_query = [timed(lambda: smap.query_dev(d_xyz.ptr, 3, k, 1, d_qrec.ptr, d_qdist.ptr, d_qcnt.ptr)) for _ in range(11)]
assert d_qrec.download(np.uint8, REC * k).tobytes() == seen[0][1], "the query at the map's own means does not find its records"
cloud_stats = {name: int(cmap.stats()[name]) for name in STAT_NAMES}
assert cloud_stats == stats, "at equal leaf the two maps hold the same voxels"

med = {key: statistics.median(v[2:]) for key, v in times.items()}
med_cloud = statistics.median(t_cloud[2:])
points = n * H * W
out = dict(source_hash=B.source_hash(), scans=n, scan_shape=[H, W], points=points, leaf=args.leaf, max_voxels=args.max_voxels, stats=stats,
           add_ms_median=dict(combined=round(med[0], 3), plain=round(med[1], 3)),
           add_ms=dict(combined=[round(t, 3) for t in times[0][2:]], plain=[round(t, 3) for t in times[1][2:]]),
           add_points_per_s=dict(combined=round(points / med[0] * 1e3), plain=round(points / med[1] * 1e3)),
           cloud_map_add_ms_median=round(med_cloud, 3), cloud_map_add_ms=[round(t, 3) for t in t_cloud[2:]],
           claims=dict(combined=claims[0], plain=claims[1], cloud_map=cmap.claims()),
           points_per_claim=dict(combined=round(stats["points_used"] / max(claims[0], 1), 3), plain=round(stats["points_used"] / max(claims[1], 1), 3)),
           atomics_per_offered_point=dict(combined=round(15 * claims[0] / max(points, 1), 3), plain=round(15 * claims[1] / max(points, 1), 3)),
           emit_ms_median=round(statistics.median(t_emit[2:]), 3), emit_ms=[round(t, 3) for t in t_emit[2:]], emit_voxels=stats["voxels"],
           query_ms_median=round(statistics.median(t_query[2:]), 3), query_ms=[round(t, 3) for t in t_query[2:]], query_points=k)
assert claims[1] == stats["points_used"], "the plain form claims once per used point"
print(json.dumps(out), flush=True)
smap.close(), cmap.close()
for b in (d_scans, d_poses, d_rec, d_xyz, d_normal, d_n, d_qrec, d_qdist, d_qcnt):
    b.free()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
