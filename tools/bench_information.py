#!/usr/bin/env python3
"""Cost of the registration information pass; writes profiles/information_bench.json. Run on a GPU box.

    python tools/bench_information.py [--pairs 256] [--reps 9] [--out profiles/information_bench.json]

1. The same resident 64 x 1024 scan pairs through loamx_register_scan_pairs_dev and through its "_info" form, alternating in
   one run, median of --reps calls after 2: the difference is one more association pass at the final poses plus the two
   information kernels.
2. The information kernels' achieved bandwidth (72 B per edge slot + 56 B per plane slot streamed once) next to the
   residual sweep's in the same run, from the per-kernel timing of the context."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from loam_amd import build as B  # noqa: E402
from loam_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=256)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "information_bench.json"))
args = ap.parse_args()

H, W, P = 64, 1024, args.pairs
ctx = capi.Context(0)
lidar, fe, reg = capi.LidarParams(H, W, 1.0, 120.0), capi.FeatureExtractionParams(), capi.RegistrationParams()
d_xyz = ctx.alloc(P * 2 * H * W * 24)
d_res, d_res_info, d_info = ctx.alloc(P * 64), ctx.alloc(P * 64), ctx.alloc(P * capi.INFORMATION_DTYPE.itemsize)
ctx.synth_scan_pairs_dev(args.seed, 0, P, H, W, 0.01, d_xyz.ptr)
ctx.synchronize()


def run(info):
    ctx.synchronize()
    t0 = time.perf_counter()
    ctx.register_scan_pairs_dev(d_xyz.ptr, P, lidar, fe, reg, d_res_info.ptr if info else d_res.ptr, d_info=d_info.ptr if info else None)
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


plain, with_info = [], []
for rep in range(args.reps + 2):
    a, b = run(False), run(True)
    if rep >= 2:
        plain.append(a), with_info.append(b)
res, res_info = d_res.download(capi.RESULT_DTYPE, P), d_res_info.download(capi.RESULT_DTYPE, P)
info = d_info.download(capi.INFORMATION_DTYPE, P)
assert res.tobytes() == res_info.tobytes(), "the _info form changed a result record"
out = dict(source_hash=B.source_hash(), pairs=P, scan=f"{H}x{W}", reps=args.reps,
           plain_ms=[round(t, 3) for t in plain], info_ms=[round(t, 3) for t in with_info],
           plain_ms_median=round(statistics.median(plain), 3), info_ms_median=round(statistics.median(with_info), 3),
           rows_per_pair_mean=round(float(np.mean(info["n_edge"].astype(np.float64) + info["n_plane"])), 1),
           smallest_eigenvalue_min_median_max=[round(float(f(info["eigenvalues"][:, 0])), 2) for f in (np.min, np.median, np.max)])
out["information_pass_ms"] = round(out["info_ms_median"] - out["plain_ms_median"], 3)

# per-kernel timing: the same two calls with the context's kernel timing on
ctx.enable_kernel_timing(True)
ctx.reset_kernel_stats()
for _ in range(3):
    run(False), run(True)
st = ctx.kernel_stats()
ctx.enable_kernel_timing(False)
# the information kernels stream every association slot of every pair once: the slots are the extracted feature counts
ecap, pcap = ctx.edge_capacity(lidar, fe), ctx.planar_capacity(lidar, fe)
d_ne, d_np = ctx.alloc(2 * P * 4), ctx.alloc(2 * P * 4)
d_e, d_p = ctx.alloc(2 * P * ecap * 24), ctx.alloc(2 * P * pcap * 24)
ctx.extract_features_batch_dev(d_xyz.ptr, 2 * P, lidar, fe, None, d_ne.ptr, d_e.ptr, None, d_np.ptr, d_p.ptr)
ctx.synchronize()
n_se, n_sp = d_ne.download(np.uint32, 2 * P)[1::2], d_np.download(np.uint32, 2 * P)[1::2]  # the source scans
info_bytes = 72.0 * float(n_se.sum()) + 56.0 * float(n_sp.sum())
ki, ks = st["information_kernel"], st["sweep_kernel"]
out["kernels"] = dict(
    information=dict(launches=ki["launches"], ms_per_launch=round(ki["total_ms"] / max(ki["launches"], 1), 4), bytes_per_launch=info_bytes,
                     achieved_GBs=round(info_bytes / (ki["total_ms"] / max(ki["launches"], 1)) / 1e6, 1) if ki["total_ms"] else None,
                     note="information_kernel + information_finish_kernel of one pass"),
    sweep=dict(launches=ks["launches"], ms_per_launch=round(ks["total_ms"] / max(ks["launches"], 1), 4),
               bytes_per_launch=round(ks["algorithmic_bytes"] / max(ks["launches"], 1)),
               achieved_GBs=round(ks["algorithmic_bytes"] / ks["total_ms"] / 1e6, 1) if ks["total_ms"] else None),
    associate_ms_per_launch=round(st["associate_kernel"]["total_ms"] / max(st["associate_kernel"]["launches"], 1), 4))
print(json.dumps(out), flush=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
