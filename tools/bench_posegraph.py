#!/usr/bin/env python3
"""Measurements of the pose-graph optimiser; writes profiles/posegraph_bench.json. Run on a GPU box.

    python tools/bench_posegraph.py [--sizes 1000 10000 100000] [--steps 9] [--warmup 2] [--out profiles/posegraph_bench.json]

Chains of n poses on a ring with 1 % loop edges, resident on the device, started from a drifted copy of the truth. Per size,
with events on the stream the context is given (a torch side stream) around one `pose_graph_optimize_dev` call, the poses put
back from a pristine copy before every call, the median of `steps`:
  solve          the call at the default parameters: ms, LM iterations, PCG iterations per solve
  lm_iteration   max_iterations = 1: ms per LM iteration with its inner solve as the defaults run it
  fixed          max_iterations = 1, max_pcg_iterations = 0: what an LM iteration costs around its inner solve (the incidence lists,
                 linearisation, gather, candidate, its cost, the decision)
  terminated_at_once  the truth with measurements composed from it (cost exactly 0): the solve ends in its first iteration; ms of
                 the call and us per enqueued launch, nearly all of which return at their first branch
  pcg            max_iterations = 1, pcg_tolerance = 0 (the inner solve runs to its cap of 500): (ms - fixed) / 500 = us per PCG
                 iteration, and the algorithmic bytes of an iteration over that time"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from loam_amd import build as B  # noqa: E402
from loam_amd import capi  # noqa: E402
import posegraph_common as G  # noqa: E402  (the numpy pose algebra that makes the graphs)

HBM_PEAK_GBS = 8000.0  # MI355X data sheet
ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 10000, 100000])
ap.add_argument("--steps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posegraph_bench.json"))
args = ap.parse_args()

import torch  # noqa: E402  (events, the stream and the buffers only)

ctx = capi.Context(0)
stream = torch.cuda.Stream()
ctx.set_stream(stream.cuda_stream)


def graph(n, seed=1):
    """n poses on a ring, odometry edges with noise, n / 100 loop edges; the start: the truth pushed off by a random walk"""
    rng = np.random.default_rng(seed)
    truth = G.ring_truth(n, radius=n / 20.0, rng=rng)
    pairs = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)
    a = rng.integers(0, n, size=n // 100)
    b = (a + rng.integers(n // 10, n - n // 10, size=len(a))) % n
    pairs = np.concatenate([pairs, np.stack([a, b], axis=1)])
    edges = G.make_edges(pairs, G.measured(truth, pairs, rng, 0.002, 0.02), np.diag([2500.0] * 3 + [400.0] * 3))
    walk = np.cumsum(np.concatenate([0.0005 * rng.normal(size=(n, 3)), 0.005 * rng.normal(size=(n, 3))], axis=1), axis=0)
    walk[0] = 0.0
    exact = G.make_edges(pairs, G.measured(truth, pairs, rng), np.diag([2500.0] * 3 + [400.0] * 3))
    return G.retract(truth, walk), edges, truth, exact


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def timed(pristine, work, d_edges, n, m, d_summary, **kw):
    """(median ms, min, max, last summary) of one call with these parameters"""
    params = capi.PgoParams(**kw)
    times = []
    for i in range(args.warmup + args.steps):
        with torch.cuda.stream(stream):
            work.copy_(pristine)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        ctx.pose_graph_optimize_dev(work.data_ptr(), n, d_edges.data_ptr(), m, 0, params, d_summary.data_ptr())
        e1.record(stream)
        e1.synchronize()
        if i >= args.warmup:
            times.append(e0.elapsed_time(e1))
    s = np.frombuffer(d_summary.cpu().numpy().tobytes(), dtype=capi.PGO_SUMMARY_DTYPE)[0]
    return statistics.median(times), min(times), max(times), s


def pcg_bytes(n, m):
    """algorithmic bytes of one PCG iteration: the SpMV reads each pose's damped block (288), z and p (96) and writes p and q
    (96), and per incidence entry (2 m of them) the entry (4), the edge's ends (8), H_ab (288) and the neighbour's z and p (96);
    the update reads the inverse block (288), p and q (96), reads and writes x and r (192) and writes z (48)"""
    return n * (288 + 96 + 96) + 2 * m * (4 + 8 + 288 + 96) + n * (288 + 96 + 192 + 48)


out = dict(source_hash=B.source_hash(), steps=args.steps, warmup=args.warmup, hbm_peak_GBs=HBM_PEAK_GBS,
           timing="events on the context's stream around one pose_graph_optimize_dev call; median of `steps`", graphs={})
for n in args.sizes:
    poses, edges, truth, exact = graph(n)
    m = len(edges)
    pristine, d_edges, d_summary = dev(poses), dev(edges), dev(np.zeros(1, capi.PGO_SUMMARY_DTYPE))
    work = pristine.clone()
    torch.cuda.synchronize()
    rec = dict(poses=n, edges=m, loop_edges=m - (n - 1))
    ms, lo, hi, s = timed(pristine, work, d_edges, n, m, d_summary)
    rec["solve"] = dict(ms=round(ms, 4), ms_min_max=[round(lo, 4), round(hi, 4)], lm_iterations=int(s["iterations"]), accepted=int(s["accepted"]),
                        pcg_iterations=int(s["pcg_iterations"]), termination=capi.PGO_TERMINATIONS[s["termination"]],
                        initial_cost=float(s["initial_cost"]), final_cost=float(s["final_cost"]))
    ms1, lo, hi, s = timed(pristine, work, d_edges, n, m, d_summary, max_iterations=1)
    rec["lm_iteration"] = dict(ms=round(ms1, 4), ms_min_max=[round(lo, 4), round(hi, 4)], pcg_iterations=int(s["pcg_iterations"]))
    ms0, lo, hi, s = timed(pristine, work, d_edges, n, m, d_summary, max_iterations=1, max_pcg_iterations=0)
    rec["fixed"] = dict(ms=round(ms0, 4), ms_min_max=[round(lo, 4), round(hi, 4)])
    msp, lo, hi, s = timed(pristine, work, d_edges, n, m, d_summary, max_iterations=1, pcg_tolerance=0.0)
    its = int(s["pcg_iterations"])
    us = (msp - ms0) * 1e3 / max(its, 1)
    rec["pcg"] = dict(ms=round(msp, 4), ms_min_max=[round(lo, 4), round(hi, 4)], pcg_iterations=its, us_per_pcg_iteration=round(us, 3),
                      algorithmic_bytes_per_iteration=pcg_bytes(n, m), GBs=round(pcg_bytes(n, m) / (us * 1e-6) / 1e9, 1),
                      fraction_of_hbm_peak=round(pcg_bytes(n, m) / (us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4))
    # the truth with measurements composed from it: the cost is exactly 0, the solve ends in its first iteration, and every
    # launch enqueued behind that returns at its first branch
    ms_i, lo, hi, s = timed(dev(truth), work, dev(exact), n, m, d_summary)
    launches = 5 + 20 * (5 + 2 * min(500, 6 * n)) + 1
    rec["terminated_at_once"] = dict(ms=round(ms_i, 4), ms_min_max=[round(lo, 4), round(hi, 4)], lm_iterations=int(s["iterations"]),
                                     termination=capi.PGO_TERMINATIONS[s["termination"]], launches_enqueued=launches,
                                     us_per_launch=round(ms_i * 1e3 / launches, 3))
    out["graphs"]["N%d" % n] = rec
    print(json.dumps({("N%d" % n): rec}), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print("wrote", args.out)
