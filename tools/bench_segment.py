#!/usr/bin/env python3
"""Measurements of the scan segmentation; writes profiles/segment_bench.json. Run on a GPU box.

    python tools/bench_segment.py [--scans 256] [--out profiles/segment_bench.json]

`--scans` resident 64 x 1024 scans of the parking lot and of the canyon of tests/outdoor_scenes.py (as many different sensor poses
along a drive; --distinct fewer, repeated), float64 and float32 input, one loamx_segment_scans_dev call with every output
written: the tile form and the global-only form (context option NO_SEGMENT_TILES) alternating in one process on the same
inputs, events on the context's stream, median of 9 after 2; both forms must leave the same bytes. In the same run the de-skew
kernel over the same scans (it reads and writes every point once: the bandwidth yardstick). Algorithmic bytes per cell of the
segmentation: the point read once, classes + labels + sizes + the filtered point written once."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import outdoor_scenes as S  # noqa: E402
from loam_amd import build as B  # noqa: E402
from loam_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scans", type=int, default=256)
ap.add_argument("--distinct", type=int, default=256, help="different sensor poses per scene")
ap.add_argument("--steps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_bench.json"))
args = ap.parse_args()
import torch  # noqa: E402  (events and the stream only)

ctx = capi.Context(0)
stream = torch.cuda.Stream()
ctx.set_stream(stream.cuda_stream)
H, W, n = 64, 1024, args.scans
HW = H * W
lidar = capi.LidarParams(H, W, 1.0, 120.0)
params = capi.SegmentParams()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def drive(scene):
    o0, yaw0 = S.sensor_origin(scene, 0)
    step = 0.8 if scene == "canyon" else 0.1
    scans = [S.scan_at(scene, 0, o0 + step * i * np.array([np.cos(yaw0), np.sin(yaw0), 0.0]), yaw0 + 0.006 * i, H, W, 0.01, noise_seed=1000 + i)
             for i in range(min(args.distinct, n))]
    return np.ascontiguousarray([scans[i % len(scans)] for i in range(n)])


out = dict(source_hash=B.source_hash(), scans=n, distinct_scans=min(args.distinct, n), scan_shape=[H, W], steps=args.steps, warmup=args.warmup,
           timing="events on the context's stream around one call; the two forms alternate; median of `steps` after `warmup`", cases={})
for scene in ("lot", "canyon"):
    scans64 = drive(scene)
    for f32 in (False, True):
        scans = scans64.astype(np.float32) if f32 else scans64
        scalar = 4 if f32 else 8
        d_in = ctx.alloc(scans.nbytes).upload(scans)
        bufs = dict(classes=ctx.alloc(n * HW), labels=ctx.alloc(4 * n * HW), sizes=ctx.alloc(4 * n * HW), filtered=ctx.alloc(scans.nbytes),
                    clusters=ctx.alloc(16 * n * 4096), stats=ctx.alloc(32 * n), motion=ctx.alloc(56 * n))
        bufs["motion"].upload(np.tile(np.array([0.0, 0.0, 0.002, 1.0, 0.3, 0.01, 0.0]), (n, 1)))

        def call():
            ctx.segment_scans_dev(d_in.ptr, n, lidar, params, bufs["classes"].ptr, bufs["labels"].ptr, bufs["sizes"].ptr, bufs["filtered"].ptr,
                                  bufs["clusters"].ptr, 4096, bufs["stats"].ptr, f32=f32)

        times, seen, census = {0: [], 1: []}, {}, {}
        for rep in range(args.warmup + args.steps):
            for no_tiles in (0, 1):
                ctx.set_option("NO_SEGMENT_TILES", no_tiles)
                times[no_tiles].append(timed(call))
                if rep == 0:
                    census[no_tiles] = ctx.last_segment_census()
                    seen[no_tiles] = tuple(bufs[k].download(np.uint8, bufs[k].nbytes).tobytes() for k in ("classes", "labels", "sizes", "filtered", "stats"))
        ctx.set_option("NO_SEGMENT_TILES", 0)
        assert seen[0] == seen[1], "the two forms left different bytes"
        stats = np.frombuffer(seen[0][4], np.uint32).reshape(n, 8).astype(np.int64)
        t_deskew = [timed(lambda: ctx.deskew_scans_dev(d_in.ptr, n, lidar, bufs["motion"].ptr, bufs["filtered"].ptr, 1.0, f32=f32))
                    for _ in range(args.warmup + args.steps)]
        med = {k: statistics.median(v[args.warmup:]) for k, v in times.items()}
        med_deskew = statistics.median(t_deskew[args.warmup:])
        bytes_per_cell = 3 * scalar + 1 + 4 + 4 + 3 * scalar
        case = dict(ms_median=dict(tiles=round(med[0], 4), global_only=round(med[1], 4)),
                    ms=dict(tiles=[round(t, 4) for t in times[0][args.warmup:]], global_only=[round(t, 4) for t in times[1][args.warmup:]]),
                    us_per_scan=dict(tiles=round(med[0] / n * 1e3, 3), global_only=round(med[1] / n * 1e3, 3)),
                    algorithmic_bytes_per_cell=bytes_per_cell,
                    algorithmic_GBs=dict(tiles=round(bytes_per_cell * n * HW / med[0] / 1e6, 1), global_only=round(bytes_per_cell * n * HW / med[1] / 1e6, 1)),
                    deskew_ms_median=round(med_deskew, 4), deskew_bytes_per_cell=6 * scalar,
                    deskew_GBs=round(6 * scalar * n * HW / med_deskew / 1e6, 1),
                    merged_edges=dict(tiles=census[0].merged_edges, global_only=census[1].merged_edges),
                    tile=[census[0].tile_lines, census[0].tile_cols], tiles_per_scan=census[0].tiles_per_scan,
                    shares=dict(invalid=round(float(stats[:, 0].sum()) / (n * HW), 4), ground=round(float(stats[:, 1].sum()) / (n * HW), 4),
                                cluster=round(float(stats[:, 2].sum()) / (n * HW), 4), outlier=round(float(stats[:, 3].sum()) / (n * HW), 4)),
                    components_per_scan=dict(accepted=round(float(stats[:, 4].mean()), 1), rejected=round(float(stats[:, 5].mean()), 1)))
        out["cases"]["%s_%s" % (scene, "f32" if f32 else "f64")] = case
        print(scene, "f32" if f32 else "f64", json.dumps(case), flush=True)
        d_in.free()
        for b in bufs.values():
            b.free()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
