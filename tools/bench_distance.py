#!/usr/bin/env python3
"""Measurements of the occupancy distance field; writes profiles/distance_bench.json. Run on a GPU box.

    python tools/bench_distance.py [--scans 256] [--leaf 0.2] [--out profiles/distance_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/bench_distance.py --trace-run
    python tools/bench_distance.py --merge-trace DIR [--out profiles/distance_bench.json]

The map is that of tools/bench_occupancy.py: `--scans` 64 x 1024 float scans of the canyon drive at leaf 0.2 m. The shapes are the
512 x 512 x 16 box of that tool and its slice, with R = 10 and 50. Per shape:
 (a) the call (loamx_occupancy_distance_box / _slice, all three outputs), median of 9 after 2, against the map's own read-out of
     the same EXTENDED box (loamx_occupancy_box_dev, states only / loamx_occupancy_slice_dev): what the lookups alone cost;
 (c) the early-exit form against the whole window (NO_DISTANCE_EARLY_EXIT), alternating in one process; both must leave the
     same bytes;
 (d) scipy.ndimage.distance_transform_edt on the same mask on the host, plus the device-to-host copy of the states it needs:
     context only (another machine, and it computes no offsets).
 (b) per launch, the algorithmic bytes (mask bits, intermediates, outputs; the table's lines are not counted) over its time: from a
     kernel trace taken in a run of its own (--trace-run under rocprofv3, then --merge-trace)."""
import argparse
import csv
import glob
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distance_bench.json"))
ap.add_argument("--trace-run", action="store_true", help="three calls per shape and form, nothing else: the run rocprofv3 traces")
ap.add_argument("--merge-trace", default=None, help="directory of a traced --trace-run: adds (b) to the file --out names")
args = ap.parse_args()

DIMS = (512, 512, 16)
RADII = (10, 50)
TRACE_CALLS = 3
SHAPES = [(kind, R) for kind in ("box", "slice") for R in RADII]


def launches(kind, R):
    """[(kernel name fragment, algorithmic bytes)] of one call with all three outputs"""
    dx, dy, dz = DIMS
    ex, ey, ez = dx + 2 * R, dy + 2 * R, (dz + 2 * R if kind == "box" else 1)
    words = ey * ez * ((ex + 63) // 64)
    n_x = ey * ez * dx
    out = [("distance_mask_kernel", words * 8), ("distance_x_kernel", words * 8 + n_x * 2)]
    if kind == "box":
        n_y, n = ez * dy * dx, dz * dy * dx
        out += [("distance_column_kernel<false, false>", n_x * 2 + n_y * 4), ("distance_column_kernel<true, true>", n_y * 4 + n * (2 + 6 + 4))]
    else:
        out += [("distance_column_kernel<false, true>", n_x * 2 + dy * dx * (2 + 4 + 4))]
    return out


def merge_trace():
    files = glob.glob(os.path.join(args.merge_trace, "**", "*_kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = [r for r in csv.DictReader(open(files[0])) if "distance_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    record = json.load(open(args.out))
    at, per_launch = 0, {}
    for kind, R in SHAPES:  # the warm-up calls of --trace-run
        for name, _ in launches(kind, R):
            assert name in rows[at]["Kernel_Name"], (name, rows[at]["Kernel_Name"], at)
            at += 1
    for kind, R in SHAPES:
        for form in ("early_exit", "whole_window"):
            ls = launches(kind, R)
            times = [[] for _ in ls]
            for _ in range(TRACE_CALLS):
                for j, (name, _) in enumerate(ls):
                    r = rows[at]
                    assert name in r["Kernel_Name"], (name, r["Kernel_Name"], at)
                    times[j].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
                    at += 1
            per_launch["%s_R%d_%s" % (kind, R, form)] = [
                dict(kernel=name, us_median=round(statistics.median(t), 2), us=[round(v, 2) for v in t], algorithmic_bytes=b,
                     gb_per_s=round(b / statistics.median(t) / 1e3, 1)) for (name, b), t in zip(ls, times)]
    assert at == len(rows), (at, len(rows))
    record["per_launch"] = per_launch
    record["per_launch_note"] = ("rocprofv3 --kernel-trace in a run of its own, %d calls per shape and form; bytes are the mask bits, intermediates and "
                                 "outputs a launch reads and writes by the algorithm, not the table's lines" % TRACE_CALLS)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(json.dumps(per_launch))


if args.merge_trace:
    merge_trace()
    sys.exit(0)

import occupancy_common as M  # noqa: E402
import outdoor_scenes as S  # noqa: E402
from loam_amd import build as B  # noqa: E402
from loam_amd import capi  # noqa: E402

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
centre = np.floor(poses[n // 2, 4:] / args.leaf).astype(np.int64)
vmin, dims = (centre - [DIMS[0] // 2, DIMS[1] // 2, DIMS[2] // 2]).astype(np.int32), np.array(DIMS, dtype=np.uint32)
n_box, n_slice = int(np.prod(DIMS)), DIMS[0] * DIMS[1]
d_d2, d_off, d_m = ctx.alloc(n_box * 2), ctx.alloc(n_box * 6), ctx.alloc(n_box * 4)
e_max = [d + 2 * max(RADII) for d in DIMS]
d_states = ctx.alloc(int(np.prod(e_max)))


def timed(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def call(kind, R):
    fn = omap.distance_box_dev if kind == "box" else omap.distance_slice_dev
    fn(vmin, dims, capi.DistanceParams(R), d_d2.ptr, d_off.ptr, d_m.ptr)


def outputs(kind):
    k = n_box if kind == "box" else n_slice
    return d_d2.download(np.uint16, k).tobytes(), d_off.download(np.int16, k * (3 if kind == "box" else 2)).tobytes(), d_m.download(np.float32, k).tobytes()


if args.trace_run:
    for kind, R in SHAPES:  # warm-up, one call per shape: the staging grows here (--merge-trace skips these launches)
        call(kind, R)
    for kind, R in SHAPES:
        for whole in (0, 1):
            ctx.set_option("NO_DISTANCE_EARLY_EXIT", whole)
            for _ in range(TRACE_CALLS):
                call(kind, R)
    ctx.synchronize()
    omap.close()
    sys.exit(0)

record = dict(source_hash=B.source_hash(), scans=n, scan_shape=[H, W], leaf=args.leaf, stats=stats, vmin=vmin.tolist(), dims=list(DIMS), shapes={})
for kind, R in SHAPES:
    ext_vmin = (vmin.astype(np.int64) - [R, R, R if kind == "box" else 0]).astype(np.int32)
    ext_dims = np.array([DIMS[0] + 2 * R, DIMS[1] + 2 * R, DIMS[2] + (2 * R if kind == "box" else 0)], dtype=np.uint32)
    readout = (lambda: omap.box_dev(ext_vmin, ext_dims, 0, d_states.ptr)) if kind == "box" else (lambda: omap.slice_dev(ext_vmin, ext_dims, d_states.ptr))
    times, seen = {0: [], 1: []}, {}
    for rep in range(11):
        for whole in (0, 1):
            ctx.set_option("NO_DISTANCE_EARLY_EXIT", whole)
            times[whole].append(timed(lambda: call(kind, R)))
            if rep == 0:
                seen[whole] = outputs(kind)
    ctx.set_option("NO_DISTANCE_EARLY_EXIT", 0)
    assert seen[0] == seen[1], "the early exit changed the field"
    t_read = [timed(readout) for _ in range(11)]
    # (d) the host's route: the states of the extended box to the host, then scipy's exact transform
    n_ext = int(np.prod(ext_dims.astype(np.int64))) if kind == "box" else int(ext_dims[0]) * int(ext_dims[1])
    t0 = time.perf_counter()
    states = d_states.download(np.uint8, n_ext)
    t_copy = (time.perf_counter() - t0) * 1e3
    from scipy.ndimage import distance_transform_edt
    free = (states != M.OCCUPIED).reshape([int(v) for v in (ext_dims[::-1] if kind == "box" else ext_dims[1::-1])])
    t0 = time.perf_counter()
    edt = distance_transform_edt(free)
    t_edt = (time.perf_counter() - t0) * 1e3
    d2 = np.frombuffer(seen[0][0], dtype=np.uint16).reshape(DIMS[::-1] if kind == "box" else DIMS[1::-1])
    inner = edt[tuple(slice(R, R + s) for s in d2.shape)]
    near = inner <= R
    assert (d2[near] == np.rint(inner[near] ** 2)).all() and (d2[~near] == capi.DIST_FAR).all(), "the field differs from scipy's"
    med = {k: statistics.median(v[2:]) for k, v in times.items()}
    read_ms = statistics.median(t_read[2:])
    record["shapes"]["%s_R%d" % (kind, R)] = dict(
        extended_dims=[int(v) for v in ext_dims], launches=len(launches(kind, R)),
        call_ms_median=dict(early_exit=round(med[0], 3), whole_window=round(med[1], 3)),
        call_ms=dict(early_exit=[round(t, 3) for t in times[0][2:]], whole_window=[round(t, 3) for t in times[1][2:]]),
        whole_over_early=round(med[1] / med[0], 3),
        readout_of_extended_box_ms_median=round(read_ms, 3), readout_ms=[round(t, 3) for t in t_read[2:]],
        call_over_readout=round(med[0] / read_ms, 3),
        host_route_ms=dict(d2h_copy=round(t_copy, 3), scipy_edt=round(t_edt, 3)),
        cells=dict(zero=int((d2 == 0).sum()), near=int(((d2 > 0) & (d2 < capi.DIST_FAR)).sum()), far=int((d2 == capi.DIST_FAR).sum())),
        algorithmic_bytes={name: b for name, b in launches(kind, R)})
    print("%s R=%d: %.3f ms early, %.3f ms whole, read-out %.3f ms" % (kind, R, med[0], med[1], read_ms), file=sys.stderr, flush=True)

print(json.dumps(record), flush=True)
omap.close()
for b in (d_scans, d_poses, d_d2, d_off, d_m, d_states):
    b.free()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(record, f, indent=1)
    f.write("\n")
