#!/usr/bin/env python3
"""Measurements of the occupancy map; writes profiles/occupancy_bench.json. Run on a GPU box.

    python tools/bench_occupancy.py [--scans 256] [--leaf 0.2] [--out profiles/occupancy_bench.json]

1. add: `--scans` resident 64 x 1024 float scans of the canyon drive of tools/bench_cloudmap.py at their ground-truth poses
   (device poses), the default parameters, one loamx_occupancy_add_clouds_dev_f32 call into a cleared map, with run combining
   and without (NO_OCCUPANCY_COMBINE), alternating in one process on the same inputs, median of 9 calls after 2; both forms
   must leave the same stats and the same bytes in a box around the drive.
2. claims: the walk kernel counts how often it began a probe (loamx_occupancy_claims_read): once per hit and per pass in the
   plain form, once per run of a wavefront with combining.
3. read-outs: a 512 x 512 x 16 box and the slice over the same voxels, median of 9 after 2.
4. the cloud map's add on the same scans in the same run, for the ratio."""
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
import occupancy_common as M  # noqa: E402
import outdoor_scenes as S  # noqa: E402
from loam_amd import build as B  # noqa: E402
from loam_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scans", type=int, default=256)
ap.add_argument("--leaf", type=float, default=0.2)
ap.add_argument("--max-voxels", type=int, default=1 << 25)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occupancy_bench.json"))
args = ap.parse_args()
ctx = capi.Context(0)
H, W, n = 64, 1024, args.scans
params = capi.OccupancyParams(leaf=args.leaf)

o0, yaw0 = S.sensor_origin("canyon", 3)
scans, poses = [], []
for i in range(n):
    origin, yaw = o0 + 0.8 * i * np.array([np.cos(yaw0), np.sin(yaw0), 0.0]), yaw0 + 0.006 * i
    scans.append(S.scan_at("canyon", 0, origin, yaw, H, W, 0.01, noise_seed=1000 + i).astype(np.float32))
    poses.append(S.yaw_pose(yaw, origin))
    if i % 32 == 31:
        print("%d scans cast" % (i + 1), file=sys.stderr, flush=True)
scans, poses = np.ascontiguousarray(scans), np.ascontiguousarray(poses)
offsets = np.arange(n + 1) * (H * W)
d_scans, d_poses = ctx.alloc(scans.nbytes).upload(scans), ctx.alloc(poses.nbytes).upload(poses)
omap = ctx.occupancy_map(params, args.max_voxels)
cmap = ctx.cloud_map(capi.CloudMapParams(leaf=args.leaf), 1 << 22)
centre = np.floor(poses[n // 2, 4:] / args.leaf).astype(np.int64)
box_vmin, box_dims = (centre - [256, 256, 8]).astype(np.int32), np.array([512, 512, 16], dtype=np.uint32)
n_box = int(np.prod(box_dims.astype(np.int64)))
d_counts, d_states, d_grid = ctx.alloc(n_box * 8), ctx.alloc(n_box), ctx.alloc(512 * 512)


def timed(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def add(plain):
    ctx.set_option("NO_OCCUPANCY_COMBINE", plain)
    omap.clear()
    return timed(lambda: omap.add_clouds_dev(d_scans.ptr, 3, offsets, d_poses.ptr, f32=True))


def cloud_add():
    cmap.clear()
    return timed(lambda: cmap.add_clouds_dev(d_scans.ptr, 3, offsets, d_poses.ptr, f32=True))


times, seen, claims = {0: [], 1: []}, {}, {}
for rep in range(11):
    for plain in (0, 1):
        times[plain].append(add(plain))
        if rep == 0:
            omap.box_dev(box_vmin, box_dims, d_counts.ptr, d_states.ptr)
            seen[plain] = ({name: int(omap.stats()[name]) for name in M.STAT_NAMES}, d_counts.download(np.uint32, 2 * n_box).tobytes())
            claims[plain] = omap.claims()
    print("rep %d: %.1f / %.1f ms" % (rep, times[0][-1], times[1][-1]), file=sys.stderr, flush=True)
assert seen[0] == seen[1], "run combining changed the map"
stats = seen[0][0]
assert stats["overflow"] == 0, "the table is too small for the drive: raise --max-voxels"
ctx.set_option("NO_OCCUPANCY_COMBINE", 0)
t_box = [timed(lambda: omap.box_dev(box_vmin, box_dims, d_counts.ptr, d_states.ptr)) for _ in range(11)]
t_slice = [timed(lambda: omap.slice_dev(box_vmin, box_dims, d_grid.ptr)) for _ in range(11)]
t_cloud = [cloud_add() for _ in range(11)]
states = d_states.download(np.uint8, n_box)

med = {k: statistics.median(v[2:]) for k, v in times.items()}
rays = n * H * W
cap = 1
while cap < 2 * args.max_voxels:
    cap *= 2
cloud_ms = statistics.median(t_cloud[2:])
out = dict(source_hash=B.source_hash(), scans=n, scan_shape=[H, W], rays=rays, leaf=args.leaf, max_voxels=args.max_voxels, stats=stats,
           params={k: getattr(params, k) for k in params.NAMES},
           add_ms_median=dict(combined=round(med[0], 3), plain=round(med[1], 3)),
           add_ms=dict(combined=[round(t, 3) for t in times[0][2:]], plain=[round(t, 3) for t in times[1][2:]]),
           plain_over_combined=round(med[1] / med[0], 3),
           rays_per_s=dict(combined=round(rays / med[0] * 1e3), plain=round(rays / med[1] * 1e3)),
           visits_per_s=dict(combined=round(stats["visits"] / med[0] * 1e3), plain=round(stats["visits"] / med[1] * 1e3)),
           claims=dict(combined=claims[0], plain=claims[1]),
           visits_and_hits_per_claim=dict(combined=round((stats["visits"] + stats["rays_hit"]) / max(claims[0], 1), 3),
                                          plain=round((stats["visits"] + stats["rays_hit"]) / max(claims[1], 1), 3)),
           visits_per_ray=round(stats["visits"] / max(rays, 1), 2), table_slots=cap, table_load=round(stats["voxels"] / cap, 4),
           box=dict(vmin=box_vmin.tolist(), dims=box_dims.tolist(), ms_median=round(statistics.median(t_box[2:]), 3),
                    ms=[round(t, 3) for t in t_box[2:]],
                    occupied=int((states == M.OCCUPIED).sum()), free=int((states == M.FREE).sum()), unknown=int((states == M.UNKNOWN).sum())),
           slice_ms_median=round(statistics.median(t_slice[2:]), 3), slice_ms=[round(t, 3) for t in t_slice[2:]],
           cloud_map_add_ms_median=round(cloud_ms, 3), add_over_cloud_map_add=round(med[0] / cloud_ms, 2))
assert claims[1] == stats["visits"] + stats["rays_hit"], "the plain form claims once per hit and per pass"
print(json.dumps(out), flush=True)
omap.close(), cmap.close()
for b in (d_scans, d_poses, d_counts, d_states, d_grid):
    b.free()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
