#!/usr/bin/env python3
"""Measurements of the map cleaning; writes profiles/visibility_bench.json. Run on a GPU box.

    python tools/bench_visibility.py [--scans 256] [--leaf 0.2] [--out profiles/visibility_bench.json]

The workload of tools/bench_cloudmap.py: `--scans` resident 64 x 1024 float scans of the canyon drive at their device poses, the
emitted centroids of their leaf-0.2 cloud map as map points, default parameters. One loamx_visibility_votes_dev_f32 call in the
form that reads squared ranges a first launch wrote (that launch is part of the call and of its time) and in the form that reads
the scans' points (context option NO_VISIBILITY_RANGES), alternating in one process on the same inputs, events on the context's stream,
median of 9 after 2; both forms must leave the same votes. Then the filter on those votes, and as a yardstick
loamx_organize_clouds_dev_f32 on one cloud of map points seen from the middle scan, repeated until it has as many points as
there were projected pairs (at most --yardstick-cap): it applies the same cell rule once per point."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import organize_common as O  # noqa: E402
import outdoor_scenes as S  # noqa: E402
import visibility_common as V  # noqa: E402
from loam_amd import build as B  # noqa: E402
from loam_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scans", type=int, default=256)
ap.add_argument("--leaf", type=float, default=0.2)
ap.add_argument("--max-voxels", type=int, default=1 << 22)
ap.add_argument("--steps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--yardstick-cap", type=int, default=1 << 26, help="most points of the organiser's cloud")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visibility_bench.json"))
args = ap.parse_args()
import torch  # noqa: E402  (events and the stream only)

ctx = capi.Context(0)
stream = torch.cuda.Stream()
ctx.set_stream(stream.cuda_stream)
H, W, n = 64, 1024, args.scans


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


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
cmap = ctx.cloud_map(capi.CloudMapParams(leaf=args.leaf), args.max_voxels)
cmap.add_clouds_dev(d_scans.ptr, 3, offsets, d_poses.ptr, f32=True)
cmap.emit_dev(d_xyz.ptr, args.max_voxels, d_n.ptr)
n_vox = int(d_n.download(np.uint32, 1)[0])
assert 0 < n_vox <= args.max_voxels, n_vox
cmap.close()

layout = ctx.scan_layout(capi.LidarParams(H, W, 1.0, 120.0), capi.OrganizeParams(elevations=O.fan_elevations(H, S.FANS["canyon"])))
params = capi.VisibilityParams()
d_votes, d_dyn, d_static, d_index, d_n_static = ctx.alloc(n_vox * 16), ctx.alloc(n_vox), ctx.alloc(n_vox * 24), ctx.alloc(n_vox * 4), ctx.alloc(4)


def votes():
    ctx.visibility_votes_dev(layout, d_xyz.ptr, 3, n_vox, d_scans.ptr, n, d_poses.ptr, d_votes.ptr, params, f32=True)


def filt():
    ctx.visibility_filter_dev(d_votes.ptr, n_vox, d_n_static.ptr, params, d_xyz.ptr, 3, d_dyn.ptr, d_static.ptr, d_index.ptr, n_vox)


times, seen, census = {0: [], 1: []}, {}, {}
for rep in range(args.warmup + args.steps):
    for form in (1, 0):
        ctx.set_option("NO_VISIBILITY_RANGES", 1 - form)
        times[form].append(timed(votes))
        if rep == 0:
            census[form] = ctx.last_visibility_census()
            seen[form] = d_votes.download(np.uint8, n_vox * 16).tobytes()
ctx.set_option("NO_VISIBILITY_RANGES", 0)
assert seen[0] == seen[1], "the two forms left different votes"
assert census[0][2:] == census[1][2:] and (census[0].form, census[1].form) == (0, 1), census
votes()
t_filter = [timed(filt) for _ in range(args.warmup + args.steps)]
n_static = int(d_n_static.download(np.uint32, 1)[0])
v = np.frombuffer(seen[0], dtype=capi.VISIBILITY_VOTES_DTYPE)
projected, in_range = census[0].projected_pairs, census[0].in_range_pairs
assert projected == sum(int(v[f].astype(np.uint64).sum()) for f in v.dtype.names)

# the yardstick: the organiser on map points in the frame of the middle scan, as many as there were projected pairs
pts = d_xyz.download(np.float64, n_vox * 3).reshape(-1, 3)
local = V.to_sensor(pts, poses[n // 2]).astype(np.float32)
r2 = (local.astype(np.float64) ** 2).sum(axis=1)
local = local[(r2 >= 1.0) & (r2 <= 6400.0)]
n_cloud = int(min(max(projected, 1), args.yardstick_cap))
cloud = np.ascontiguousarray(np.resize(local, (n_cloud, 3)))
d_cloud, d_org, d_stats = ctx.alloc(cloud.nbytes).upload(cloud), ctx.alloc(H * W * 12), ctx.alloc(16)
t_org = [timed(lambda: ctx.organize_clouds_dev(layout, d_cloud.ptr, 3, [0, n_cloud], d_org.ptr, d_stats=d_stats.ptr, f32=True))
         for _ in range(args.warmup + args.steps)]
org_stats = d_stats.download(np.uint32, 4).astype(np.int64)
org_valid = n_cloud - int(org_stats[1]) - int(org_stats[2])  # points that had a cell

med = {k: statistics.median(t[args.warmup:]) for k, t in times.items()}
med_filter, med_org = statistics.median(t_filter[args.warmup:]), statistics.median(t_org[args.warmup:])
pairs = n_vox * n
names = {0: "scans", 1: "ranges"}
ns_pair = {names[k]: med[k] * 1e6 / max(projected, 1) for k in med}
ns_org = med_org * 1e6 / max(org_valid, 1)
out = dict(source_hash=B.source_hash(), scans=n, scan_shape=[H, W], leaf=args.leaf, map_points=n_vox, pairs=pairs, steps=args.steps, warmup=args.warmup,
           timing="events on the context's stream around one call; the two forms alternate; median of `steps` after `warmup`",
           in_range_pairs=in_range, projected_pairs=projected, scan_chunks=census[0].scan_chunks,
           votes=dict((f, int(v[f].astype(np.uint64).sum())) for f in v.dtype.names),
           votes_ms_median={names[k]: round(med[k], 3) for k in med}, votes_ms={names[k]: [round(t, 3) for t in times[k][args.warmup:]] for k in times},
           pairs_per_s={names[k]: round(pairs / med[k] * 1e3) for k in med},
           ns_per_projected_pair={k: round(t, 4) for k, t in ns_pair.items()},
           default_form="ranges", scans_over_ranges=round(med[0] / med[1], 4),
           filter_ms_median=round(med_filter, 4), static_points=n_static, dynamic_points=n_vox - n_static,
           organize=dict(points=n_cloud, with_a_cell=org_valid, ms_median=round(med_org, 3), ns_per_point_with_a_cell=round(ns_org, 4)),
           votes_over_organize_per_pair={k: round(t / ns_org, 3) for k, t in ns_pair.items()})
print(json.dumps(out), flush=True)
layout.close()
for b in (d_scans, d_poses, d_xyz, d_n, d_votes, d_dyn, d_static, d_index, d_n_static, d_cloud, d_org, d_stats):
    b.free()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
