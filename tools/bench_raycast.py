#!/usr/bin/env python3
"""Measurements of the occupancy ray cast; writes profiles/raycast_bench.json. Run on a GPU box.

    python tools/bench_raycast.py [--scans 256] [--leaf 0.2] [--out profiles/raycast_bench.json]

The map is that of tools/bench_occupancy.py: `--scans` 64 x 1024 float scans of the canyon drive at leaf 0.2 m. The workload is
the whole drive rendered back: `--scans` poses x 64 x 1024 beams (capi.beam_directions of the sensor's fan) at the drive's own
poses out to the map's max_range, ranges only. Four variants alternate in one process, 2 warm-up calls and then 9 each, the
median counts:
  plain            every lane looks its own voxel up (the default form)
  combined         one look-up per run of neighbouring lanes in the same voxel (context option RAYCAST_COMBINE)
  plain_patch8x8, combined_patch8x8
                   either form with the beams handed over in an order in which 64 consecutive beams are an 8 x 8 patch of the
                   scan (8 lines x 8 columns) and not 64 columns of one line: the caller permutes d_dirs, the kernels are the same
combined and plain must leave the same bytes; the patch variants the same ranges in their own order. rays/s and visits/s (tested
visits, from the census) per variant; probes / visits is what combining saves."""
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

ap = argparse.ArgumentParser()
ap.add_argument("--scans", type=int, default=256)
ap.add_argument("--leaf", type=float, default=0.2)
ap.add_argument("--max-voxels", type=int, default=1 << 25)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raycast_bench.json"))
args = ap.parse_args()

import occupancy_common as M  # noqa: E402
import outdoor_scenes as S  # noqa: E402
from loam_amd import build as B  # noqa: E402
from loam_amd import capi  # noqa: E402

WARMUP = 2
ctx = capi.Context(0)
H, W, n = 64, 1024, args.scans
params = capi.OccupancyParams(leaf=args.leaf)
o0, yaw0 = S.sensor_origin("canyon", 3)
scans, poses = [], []
for i in range(n):
    origin, yaw = o0 + 0.8 * i * np.array([np.cos(yaw0), np.sin(yaw0), 0.0]), yaw0 + 0.006 * i
    scans.append(S.scan_at("canyon", 0, origin, yaw, H, W, 0.01, noise_seed=1000 + i).astype(np.float32))
    poses.append(S.yaw_pose(yaw, origin))
scans, poses = np.ascontiguousarray(scans), np.ascontiguousarray(poses)
offsets = np.arange(n + 1) * (H * W)
d_scans, d_poses = ctx.alloc(scans.nbytes).upload(scans), ctx.alloc(poses.nbytes).upload(poses)
omap = ctx.occupancy_map(params, args.max_voxels)
omap.add_clouds_dev(d_scans.ptr, 3, offsets, d_poses.ptr, f32=True)
stats = {name: int(omap.stats()[name]) for name in M.STAT_NAMES}
assert stats["overflow"] == 0, "the table is too small for the drive: raise --max-voxels"

top, bottom = S.FANS["canyon"]
dirs = capi.beam_directions(H, W, capi.OrganizeParams(fov_bottom=np.radians(bottom), fov_top=np.radians(top)))
# cell l W + c  ->  patch (l / 8, c / 8), inside it line-major: 64 consecutive beams are 8 lines x 8 columns
cell = np.arange(H * W).reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3).reshape(-1)
d_dirs, d_dirs_patch = ctx.alloc(dirs.nbytes).upload(dirs), ctx.alloc(dirs.nbytes).upload(np.ascontiguousarray(dirs[cell]))
n_rays = n * H * W
d_ranges = ctx.alloc(n_rays * 8)
VARIANTS = {"plain": (0, d_dirs), "combined": (1, d_dirs), "plain_patch8x8": (0, d_dirs_patch), "combined_patch8x8": (1, d_dirs_patch)}


def call(variant):
    combine, dd = VARIANTS[variant]
    ctx.set_option("RAYCAST_COMBINE", combine)
    omap.render_scans_dev(dd.ptr, H * W, d_poses.ptr, n, params.max_range, d_ranges_out=d_ranges.ptr)


def timed(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


times, census, ranges = {v: [] for v in VARIANTS}, {}, {}
for rep in range(WARMUP + args.reps):
    for v in VARIANTS:
        times[v].append(timed(lambda: call(v)))
        if rep == 0:
            census[v] = {k: int(x) for k, x in zip(capi.RAYCAST_CENSUS_DTYPE.names, ctx.last_raycast_census().tolist())}
            ranges[v] = d_ranges.download(np.float64, n_rays).reshape(n, H * W)
        print("%s rep %d: %.2f ms" % (v, rep, times[v][-1]), file=sys.stderr, flush=True)
ctx.set_option("RAYCAST_COMBINE", 0)
assert ranges["combined"].tobytes() == ranges["plain"].tobytes(), "the two forms differ"
for v in ("plain_patch8x8", "combined_patch8x8"):
    assert ranges[v].tobytes() == np.ascontiguousarray(ranges["plain"][:, cell]).tobytes(), "the patch order changed a range"
assert all(c["visits"] == census["plain"]["visits"] for c in census.values())
assert census["plain"]["probes"] == census["plain"]["visits"] == census["plain_patch8x8"]["probes"]

record = dict(source_hash=B.source_hash(), scans=n, scan_shape=[H, W], leaf=args.leaf, max_range=params.max_range, stats=stats, rays=n_rays,
              method="host wall clock around one render_scans_dev call (ranges only) with a stream synchronisation on either side; the variants "
                     "alternate in one process, %d warm-up calls then %d, the median counts" % (WARMUP, args.reps),
              returns=dict(hit=int((ranges["combined"] > 0).sum())), variants={})
for v in VARIANTS:
    t = times[v][WARMUP:]
    med = statistics.median(t)
    c = census[v]
    record["variants"][v] = dict(ms_median=round(med, 3), ms=[round(x, 3) for x in t], rays_per_s=round(n_rays / med * 1e3), visits_per_s=round(c["visits"] / med * 1e3),
                                 probes_over_visits=round(c["probes"] / c["visits"], 4), census=c)
for v in VARIANTS:
    record["variants"][v]["over_plain"] = round(record["variants"][v]["ms_median"] / record["variants"]["plain"]["ms_median"], 3)
print(json.dumps(record), flush=True)
omap.close()
for b in (d_scans, d_poses, d_dirs, d_dirs_patch, d_ranges):
    b.free()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(record, f, indent=1)
    f.write("\n")
