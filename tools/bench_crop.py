#!/usr/bin/env python3
"""Measurements of the map window; writes profiles/crop_bench.json. Run on a GPU box.

    python tools/bench_crop.py [--scans 256] [--half 100] [--out profiles/crop_bench.json]

The workload of tools/bench_surfel.py, tools/bench_cloudmap.py and tools/bench_occupancy.py: `--scans` resident 64 x 1024 float scans
of the canyon drive at their ground-truth poses (device poses), assembled into a surfel map (leaf 0.5), a cloud map (leaf 0.2) and
an occupancy map (leaf 0.2). Per map, alternating in one process on the same inputs, median of 9 after 2 (the first takes the
handle's allocation):
1. crop: the map is rebuilt from all scans (not timed), then ONE crop to +-`--half` metres in x and y around the last scan's pose,
   which lies in device memory; host clock around the call and a synchronise.
2. the partner: what a caller has to do without a crop: clear, then add again the scans whose sensor position lies in the window.
   That is a different result (`first`, the order, and the points of kept scans outside the window all differ), so the comparison
   is of cost only.
Bytes: what the algorithm has to move (flags + gather + reset + scatter, the formulas below), over the time of the whole call."""
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
ap.add_argument("--half", type=float, default=100.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crop_bench.json"))
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
offsets = np.arange(n + 1) * (H * W)
d_scans, d_poses, d_counts = ctx.alloc(scans.nbytes).upload(scans), ctx.alloc(poses.nbytes).upload(poses), ctx.alloc(16)
lo, hi = [-args.half, -args.half, -np.inf], [args.half, args.half, np.inf]
centre = poses[n - 1, 4:7]
inside = np.flatnonzero((np.abs(poses[:, 4:6] - centre[:2]) <= args.half).all(axis=1))
first_in = int(inside[0])
assert len(inside) == n - first_in, "the scans of the window are the tail of the drive"

MAPS = {  # name -> (map, 64-bit payload words of a slot, whether the map has a list with first and count)
    "surfel_map": (ctx.surfel_map(capi.SurfelMapParams(leaf=0.5), 1 << 21), 12, True),
    "cloud_map": (ctx.cloud_map(capi.CloudMapParams(leaf=0.2), 1 << 22), 3, True),
    "occupancy": (ctx.occupancy_map(capi.OccupancyParams(leaf=0.2), 1 << 25), 1, False),
}


def timed(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def table_slots(max_voxels):
    cap = 16
    while cap < 2 * max_voxels:
        cap *= 2
    return cap


def algorithmic_bytes(voxels, kept, max_voxels, words, listed):
    """flags: key (+ list entry) of every voxel read, one flag per entry written; gather: the kept records read and staged; reset: the
    table arrays written once; scatter: the staged records read and written (+ the list entry)"""
    cap = table_slots(max_voxels)
    rec = 8 + 8 * words + (8 if listed else 0)
    entries = max_voxels if listed else cap
    flags = (voxels * 12 + entries) if listed else (cap * 8 + entries)
    return dict(flags=flags, gather=2 * kept * rec, reset=cap * rec, scatter=2 * kept * rec + (4 * kept if listed else 0))


out = dict(source_hash=B.source_hash(), scans=n, scan_shape=[H, W], half_window_m=args.half, scans_in_window=len(inside), maps={})
for name, (m, words, listed) in MAPS.items():
    t_crop, t_partner, counts, before = [], [], None, None
    for rep in range(11):
        m.clear()
        m.add_clouds_dev(d_scans.ptr, 3, offsets, d_poses.ptr, f32=True)
        if rep == 0:
            before = int(m.stats()["voxels"])
            assert int(m.stats()["overflow"]) == 0, name
        t_crop.append(timed(lambda: m.crop_dev(lo, hi, d_poses.ptr + (n - 1) * 56, d_counts.ptr)))
        c = [int(v) for v in d_counts.download(np.uint32, 4)]
        assert counts in (None, c) and c[2] == 0 and c[0] + c[1] == before and int(m.stats()["voxels"]) == c[0], (name, c, before)
        counts = c

        def partner():
            m.clear()
            m.add_clouds_dev(d_scans.ptr, 3, offsets[first_in:], d_poses.ptr + first_in * 56, f32=True)
        t_partner.append(timed(partner))
    partner_voxels = int(m.stats()["voxels"])
    med_crop, med_partner = statistics.median(t_crop[2:]), statistics.median(t_partner[2:])
    parts = algorithmic_bytes(before, counts[0], m.max_voxels, words, listed)
    total = sum(parts.values())
    out["maps"][name] = dict(leaf=m.params.leaf, max_voxels=m.max_voxels, table_slots=table_slots(m.max_voxels), voxels_before=before, kept=counts[0],
                             removed=counts[1], kept_fraction=round(counts[0] / max(before, 1), 4), first_crop_ms=round(t_crop[0], 3),
                             crop_ms_median=round(med_crop, 3), crop_ms=[round(t, 3) for t in t_crop[2:]],
                             clear_and_readd_ms_median=round(med_partner, 3), clear_and_readd_ms=[round(t, 3) for t in t_partner[2:]],
                             clear_and_readd_voxels=partner_voxels, algorithmic_bytes=parts, algorithmic_bytes_total=total,
                             achieved_bytes_per_s=round(total / med_crop * 1e3))
    m.close()
print(json.dumps(out), flush=True)
for b in (d_scans, d_poses, d_counts):
    b.free()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
