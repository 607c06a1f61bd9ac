#!/usr/bin/env python3
"""Measurements of the surfel localisation; writes profiles/localize_bench.json. Run on a GPU box.

    python tools/bench_localize.py [--scans 256] [--leaf 0.5] [--out profiles/localize_bench.json]

The workload of tools/bench_surfel.py: `--scans` resident 64 x 1024 float scans of the canyon drive and the surfel map of all of
them at their ground-truth poses. One loamx_surfel_localizer_run_f32 call places every scan from its true pose displaced by 0.2 m and
1.5 degrees (fixed seed), with the plane cache and without (NO_LOCALIZE_PLANES), alternating in one process on the same inputs,
median of 9 calls after 2; both forms must leave the same bytes. An evaluation is one pass of one cloud's points (a cloud that
stops after k iterations has k + 1: the last is the pass at the returned pose)."""
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
import localize_common as L  # noqa: E402
import outdoor_scenes as S  # noqa: E402
from loam_amd import build as B  # noqa: E402
from loam_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scans", type=int, default=256)
ap.add_argument("--leaf", type=float, default=0.5)
ap.add_argument("--max-voxels", type=int, default=1 << 21)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize_bench.json"))
args = ap.parse_args()
ctx = capi.Context(0)
H, W, n = 64, 1024, args.scans

o0, yaw0 = S.sensor_origin("canyon", 3)
scans, poses = [], []
for i in range(n):
    origin, yaw = o0 + 0.8 * i * np.array([np.cos(yaw0), np.sin(yaw0), 0.0]), yaw0 + 0.006 * i
    scans.append(S.scan_at("canyon", 0, origin, yaw, H, W, 0.01, noise_seed=1000 + i).astype(np.float32))
    poses.append(S.yaw_pose(yaw, origin))
scans, poses = np.ascontiguousarray(scans), np.ascontiguousarray(poses)
start = np.ascontiguousarray(np.stack([L.displaced(poses[i], 0.2, 1.5, seed=i) for i in range(n)]))
offsets = np.arange(n + 1) * (H * W)
d_scans, d_poses, d_start = ctx.alloc(scans.nbytes).upload(scans), ctx.alloc(poses.nbytes).upload(poses), ctx.alloc(start.nbytes).upload(start)
d_out, d_res, d_info = ctx.alloc(start.nbytes), ctx.alloc(128 * n), ctx.alloc(696 * n)
smap = ctx.surfel_map(capi.SurfelMapParams(leaf=args.leaf), args.max_voxels)
smap.add_clouds_dev(d_scans.ptr, 3, offsets, d_poses.ptr, f32=True)
ctx.synchronize()
stats = {name: int(smap.stats()[name]) for name in capi.SURFEL_MAP_STATS_DTYPE.names}
assert stats["overflow"] == 0, "the map is too small for the drive: raise --max-voxels"
loc = smap.localizer(n, n * H * W)
params = capi.LocalizeParams()


def run(plain):
    ctx.set_option("NO_LOCALIZE_PLANES", plain)
    ctx.synchronize()
    t0 = time.perf_counter()
    loc.run_dev(d_scans.ptr, 3, offsets, d_start.ptr, d_out.ptr, d_res.ptr, d_info.ptr, params, f32=True)
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


times, seen = {0: [], 1: []}, {}
for rep in range(11):
    for plain in (0, 1):
        times[plain].append(run(plain))
        if rep == 0:
            seen[plain] = (d_out.download(np.uint8, start.nbytes).tobytes(), d_res.download(np.uint8, 128 * n).tobytes(),
                           d_info.download(np.uint8, 696 * n).tobytes())
ctx.set_option("NO_LOCALIZE_PLANES", 0)
assert seen[0] == seen[1], "the plane cache changed the result"
res = np.frombuffer(seen[0][1], dtype=capi.LOCALIZE_RESULT_DTYPE)
got = np.frombuffer(seen[0][0], dtype=np.float64).reshape(n, 7)
err = np.array([L.pose_error(got[i], poses[i]) for i in range(n)])
err0 = np.array([L.pose_error(start[i], poses[i]) for i in range(n)])

med = {k: statistics.median(v[2:]) for k, v in times.items()}
evaluations = int((res["iterations"].astype(np.int64) + 1).sum())
launched = params.max_iterations + 1
out = dict(source_hash=B.source_hash(), scans=n, scan_shape=[H, W], points=n * H * W, leaf=args.leaf, map_voxels=stats["voxels"],
           displaced_by=dict(metres=0.2, degrees=1.5),
           call_ms_median=dict(planes=round(med[0], 3), plain=round(med[1], 3)),
           call_ms=dict(planes=[round(t, 3) for t in times[0][2:]], plain=[round(t, 3) for t in times[1][2:]]),
           cloud_evaluations=evaluations, evaluations_launched=launched,
           ms_per_cloud_evaluation=dict(planes=round(med[0] / evaluations, 5), plain=round(med[1] / evaluations, 5)),
           points_per_s=dict(planes=round(evaluations * H * W / med[0] * 1e3), plain=round(evaluations * H * W / med[1] * 1e3)),
           rows_per_point=round(float(res["n_rows"].sum()) / (n * H * W), 4),
           iterations_histogram={str(k): int(v) for k, v in enumerate(np.bincount(res["iterations"])) if v},
           terminations={str(k): int(v) for k, v in enumerate(np.bincount(res["termination"])) if v},
           scans_with_every_direction_used=int((res["used_mask"] == 63).sum()),
           error_before=dict(metres_median=round(float(np.median(err0[:, 0])), 4), degrees_median=round(float(np.median(err0[:, 1])), 4)),
           error_after=dict(metres_median=round(float(np.median(err[:, 0])), 4), metres_max=round(float(err[:, 0].max()), 4),
                            degrees_median=round(float(np.median(err[:, 1])), 4), degrees_max=round(float(err[:, 1].max()), 4)))
print(json.dumps(out), flush=True)
loc.close(), smap.close()
for b in (d_scans, d_poses, d_start, d_out, d_res, d_info):
    b.free()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
