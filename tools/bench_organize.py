#!/usr/bin/env python3
"""Measurements of the cloud organiser; writes profiles/organize_bench.json. Run on a GPU box.

    python tools/bench_organize.py [--batch 256] [--steps 9] [--warmup 2] [--out profiles/organize_bench.json]

Resident clouds of 64 x 1024 and 128 x 2048 shape (synthetic scans of the library's generator, every cloud shuffled on its own,
all points kept), `batch` clouds per call, float64 and float32, with ring numbers and without, both keep rules. Timed with
events on the stream the context is given (a torch side stream), several calls between two events; per case: time per cloud,
bytes/s over the algorithmic bytes (organize_kernels.hip's header: what the kernels must read and write per point and per
cell), and the de-skew kernel on the same scans in the same run as the yardstick: a streaming kernel of the same shape."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from loam_amd import build as B  # noqa: E402
from loam_amd import capi  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X data sheet
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--steps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--calls", type=int, default=4, help="calls between two events")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "organize_bench.json"))
args = ap.parse_args()
if args.batch < 2 or args.batch % 2:
    ap.error("--batch must be even (the generator makes scan pairs)")

import torch  # noqa: E402  (events and the stream only)

ctx = capi.Context(0)
stream = torch.cuda.Stream()
ctx.set_stream(stream.cuda_stream)


def event_ms(fn):
    """median, min, max over `steps` of the time of `calls` calls, per call"""
    times = []
    for i in range(args.warmup + args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.calls):
            fn()
        e1.record(stream)
        e1.synchronize()
        if i >= args.warmup:
            times.append(e0.elapsed_time(e1) / args.calls)
    return statistics.median(times), min(times), max(times)


def algorithmic_bytes(n_points, cells, filled, scalar, rings, nearest, at_minimum):
    per_point = 3 * scalar + (2 if rings else 0) + (8 + 4 + 4 + 3 * scalar if nearest else 4)
    per_cell = (12 if nearest else 4) + 4 + 3 * scalar + 4
    return n_points * per_point + (4 * at_minimum if nearest else 0) + cells * per_cell + filled * 3 * scalar


out = dict(source_hash=B.source_hash(), batch=args.batch, steps=args.steps, warmup=args.warmup, calls_per_event_pair=args.calls,
           timing="events on the context's stream around `calls_per_event_pair` calls; median of `steps`", hbm_peak_GBs=HBM_PEAK_GBS, shapes={})
for H, W in ((64, 1024), (128, 2048)):
    N, n = H * W, args.batch
    lidar = capi.LidarParams(H, W, 1.0, 120.0)
    d_scans = ctx.alloc(n * N * 24)
    ctx.synth_scan_pairs_dev(11, 0, n // 2, H, W, 0.01, d_scans.ptr)  # (n / 2 pairs: n scans)
    ctx.synchronize()
    scans = d_scans.download(np.float64, n * N * 3).reshape(n, N, 3)
    rng = np.random.default_rng(3)
    clouds, rings = np.empty_like(scans), np.empty((n, N), dtype=np.uint16)
    for i in range(n):
        perm = rng.permutation(N)
        clouds[i], rings[i] = scans[i][perm], (perm // W).astype(np.uint16)
    offsets = np.arange(n + 1, dtype=np.uint64) * N
    d_rings = ctx.alloc(rings.nbytes).upload(rings)
    d_src, d_stats = ctx.alloc(n * N * 4), ctx.alloc(n * 16)
    # the generator's fan: linear in [-22.5, 22.5] degrees
    fov = (np.radians(-22.5), np.radians(22.5))
    shape = {}
    for name, dt in (("f64", np.float64), ("f32", np.float32)):
        data = np.ascontiguousarray(clouds.astype(dt))
        d_in, d_out = ctx.alloc(data.nbytes).upload(data), ctx.alloc(data.nbytes)
        f32 = dt == np.float32
        for keep_name, keep in (("keep_first", capi.ORGANIZE_KEEP_FIRST), ("keep_nearest", capi.ORGANIZE_KEEP_NEAREST)):
            lay = ctx.scan_layout(lidar, capi.OrganizeParams(keep=keep, fov_bottom=fov[0], fov_top=fov[1]))
            for with_rings in (False, True):
                call = lambda: ctx.organize_clouds_dev(lay, d_in.ptr, 3, offsets, d_out.ptr, d_rings=d_rings.ptr if with_rings else 0,  # noqa: E731
                                                       d_src_idx=d_src.ptr, d_stats=d_stats.ptr, f32=f32)
                ms, lo, hi = event_ms(call)
                ctx.synchronize()
                stats = d_stats.download(np.uint32, n * 4).reshape(n, 4).astype(np.int64)
                filled = int(stats[:, 0].sum())
                nbytes = algorithmic_bytes(n * N, n * N, filled, data.itemsize, with_rings, keep == capi.ORGANIZE_KEEP_NEAREST, filled)
                gbs = nbytes / ms / 1e6
                shape["%s_%s_%s" % (name, keep_name, "rings" if with_rings else "no_rings")] = dict(
                    ms_per_call=round(ms, 4), ms_min_max=[round(lo, 4), round(hi, 4)], us_per_cloud=round(ms / n * 1e3, 3),
                    algorithmic_bytes_per_cloud=int(nbytes // n), GBs=round(gbs, 1), fraction_of_hbm_peak=round(gbs / HBM_PEAK_GBS, 4),
                    points_per_s=round(n * N / ms * 1e3), filled=filled, invalid=int(stats[:, 1].sum()), outside=int(stats[:, 2].sum()),
                    collisions=int(stats[:, 3].sum()))
                print(H, W, name, keep_name, "rings" if with_rings else "no rings", json.dumps(shape["%s_%s_%s" % (name, keep_name, "rings" if with_rings else "no_rings")]),
                      flush=True)
            lay.close()
        # the yardstick: the de-skew kernel over the same number of points, same run
        motions = np.zeros((n, 7))
        ang = np.random.default_rng(5).uniform(0.002, 0.02, n)
        motions[:, 2], motions[:, 3], motions[:, 4] = np.sin(ang / 2), np.cos(ang / 2), 0.8
        d_m = ctx.alloc(motions.nbytes).upload(motions)
        ms, lo, hi = event_ms(lambda: ctx.deskew_scans_dev(d_in.ptr, n, lidar, d_m.ptr, d_out.ptr, 1.0, f32=f32))
        gbs = n * N * 6 * data.itemsize / ms / 1e6
        shape["%s_deskew_yardstick" % name] = dict(ms_per_call=round(ms, 4), ms_min_max=[round(lo, 4), round(hi, 4)], bytes_per_point=6 * data.itemsize,
                                                   GBs=round(gbs, 1), fraction_of_hbm_peak=round(gbs / HBM_PEAK_GBS, 4))
        print(H, W, name, "deskew", json.dumps(shape["%s_deskew_yardstick" % name]), flush=True)
        for b in (d_in, d_out, d_m):
            b.free()
    for k in [k for k in shape if not k.endswith("yardstick")]:
        shape[k]["GBs_over_deskew_GBs"] = round(shape[k]["GBs"] / shape[k[:3] + "_deskew_yardstick"]["GBs"], 3)
    out["shapes"]["%dx%d" % (H, W)] = shape
    for b in (d_scans, d_rings, d_src, d_stats):
        b.free()

with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print("wrote", args.out)
