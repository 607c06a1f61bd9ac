#!/usr/bin/env python3
"""Measurements of place recognition; writes profiles/place_bench.json. Run on a GPU box.

    python tools/bench_place.py [--batch 256] [--steps 9] [--warmup 2] [--out profiles/place_bench.json]

Descriptors: `batch` resident 64 x 1024 scans (synthetic scans of the library's generator) per call at the default 20 x 60
shape, float64 and float32: time per scan, bytes/s over the algorithmic bytes (place_kernels.hip's header), and the de-skew kernel
on the same scans in the same run as the yardstick. Searches: 1, 16 and 256 queries against 10 000 and 100 000 entries (random
descriptors with the fill of a real one) at K = 10 and 50. Timed with events on the stream the context is given (a torch side
stream), several calls between two events; the median of `steps`."""
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
ap.add_argument("--entries", type=int, nargs="+", default=[10000, 100000])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "place_bench.json"))
args = ap.parse_args()
if args.batch < 2 or args.batch % 2:
    ap.error("--batch must be even (the generator makes scan pairs)")

import torch  # noqa: E402  (events and the stream only)

ctx = capi.Context(0)
stream = torch.cuda.Stream()
ctx.set_stream(stream.cuda_stream)


def event_ms(fn, calls):
    """median, min, max over `steps` of the time of `calls` calls, per call"""
    times = []
    for i in range(args.warmup + args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(calls):
            fn()
        e1.record(stream)
        e1.synchronize()
        if i >= args.warmup:
            times.append(e0.elapsed_time(e1) / calls)
    return statistics.median(times), min(times), max(times)


out = dict(source_hash=B.source_hash(), batch=args.batch, steps=args.steps, warmup=args.warmup, calls_per_event_pair=args.calls,
           timing="events on the context's stream around `calls_per_event_pair` calls; median of `steps`", hbm_peak_GBs=HBM_PEAK_GBS,
           descriptors={}, search={})
db = ctx.place_db()
R, S = db.n_rings, db.n_sectors

# ---- descriptors of resident scans ------------------------------------------------------------------------------------
H, W = 64, 1024
N, n = H * W, args.batch
lidar = capi.LidarParams(H, W, 1.0, 120.0)
d_scans = ctx.alloc(n * N * 24)
ctx.synth_scan_pairs_dev(11, 0, n // 2, H, W, 0.01, d_scans.ptr)
ctx.synchronize()
scans = d_scans.download(np.float64, n * N * 3).reshape(n, N, 3)
d_scans.free()
offsets = np.arange(n + 1, dtype=np.uint64) * N
d_desc = ctx.alloc(n * R * S * 2)
for name, dt in (("f64", np.float64), ("f32", np.float32)):
    data = np.ascontiguousarray(scans.astype(dt))
    d_in, d_out = ctx.alloc(data.nbytes).upload(data), ctx.alloc(data.nbytes)
    f32 = dt == np.float32
    ms, lo, hi = event_ms(lambda: db.descriptors_dev(d_in.ptr, 3, offsets, d_desc.ptr, f32=f32), args.calls)
    ctx.synchronize()
    desc = d_desc.download(np.uint16, n * R * S).reshape(n, R, S)
    nbytes = n * N * 3 * data.itemsize + n * R * S * (4 + 4 + 2)
    gbs = nbytes / ms / 1e6
    rec = dict(ms_per_call=round(ms, 4), ms_min_max=[round(lo, 4), round(hi, 4)], us_per_scan=round(ms / n * 1e3, 3),
               algorithmic_bytes_per_scan=int(nbytes // n), GBs=round(gbs, 1), fraction_of_hbm_peak=round(gbs / HBM_PEAK_GBS, 4),
               points_per_s=round(n * N / ms * 1e3), filled_cells_per_scan=round(float((desc != 0).sum()) / n, 1))
    motions = np.zeros((n, 7))
    ang = np.random.default_rng(5).uniform(0.002, 0.02, n)
    motions[:, 2], motions[:, 3], motions[:, 4] = np.sin(ang / 2), np.cos(ang / 2), 0.8
    d_m = ctx.alloc(motions.nbytes).upload(motions)
    ms, lo, hi = event_ms(lambda: ctx.deskew_scans_dev(d_in.ptr, n, lidar, d_m.ptr, d_out.ptr, 1.0, f32=f32), args.calls)
    ygbs = n * N * 6 * data.itemsize / ms / 1e6
    rec["deskew_yardstick"] = dict(ms_per_call=round(ms, 4), ms_min_max=[round(lo, 4), round(hi, 4)], bytes_per_point=6 * data.itemsize,
                                   GBs=round(ygbs, 1), fraction_of_hbm_peak=round(ygbs / HBM_PEAK_GBS, 4))
    rec["GBs_over_deskew_GBs"] = round(gbs / ygbs, 3)
    out["descriptors"]["%dx%d_%s" % (H, W, name)] = rec
    print("descriptors", name, json.dumps(rec), flush=True)
    for b in (d_in, d_out, d_m):
        b.free()
d_desc.free()

# ---- searches ----------------------------------------------------------------------------------------------------------
rng = np.random.default_rng(7)
have = 0
d_q = ctx.alloc(256 * R * S * 2)
d_res = ctx.alloc(256 * 64 * capi.PLACE_MATCH_DTYPE.itemsize)
queries = rng.integers(1, 600, (256, R, S)).astype(np.uint16)
queries[rng.random(queries.shape) > 0.35] = 0
d_q.upload(queries)
for n_entries in sorted(args.entries):
    while have < n_entries:  # (random descriptors, 35 % of the cells filled, added in slabs)
        m = min(20000, n_entries - have)
        d = rng.integers(1, 600, (m, R, S)).astype(np.uint16)
        d[rng.random(d.shape) > 0.35] = 0
        db.add(d)
        have += m
    for n_queries in (1, 16, 256):
        for K in (10, 50):
            calls = args.calls if n_queries * n_entries < 4e6 else 1
            ms, lo, hi = event_ms(lambda: db.search_dev(d_q.ptr, n_queries, K, d_res.ptr), calls)
            ctx.synchronize()
            key_bytes = n_queries * n_entries * 4 * R
            shift_bytes = n_queries * K * 2 * (2 * R * S + 8 * S)
            rec = dict(ms_per_call=round(ms, 4), ms_min_max=[round(lo, 4), round(hi, 4)], us_per_query=round(ms / n_queries * 1e3, 2),
                       key_stage_bytes=key_bytes, shift_stage_bytes=shift_bytes, key_pairs_per_s=round(n_queries * n_entries / ms * 1e3),
                       column_dots_per_call=n_queries * K * S * S)
            out["search"]["N%d_Q%d_K%d" % (n_entries, n_queries, K)] = rec
            print("search", n_entries, n_queries, K, json.dumps(rec), flush=True)
d_q.free(), d_res.free()
db.close()

with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print("wrote", args.out)
