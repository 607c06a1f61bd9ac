#!/usr/bin/env python3
"""Measurements of the map upkeep entry points; writes profiles/map_bench.json. Run on a GPU box.

    python tools/bench_map.py [--drive-scans 257] [--out profiles/map_bench.json] [--only insert|filter|drive]

1. insert: one 128 x 2048 scan's features (~39 k planar + ~8 k edge) into the config-5 map (1.02 M planar points, as
   tools/extra_configs.py builds it): loamx_target_index_insert_filtered against the plain loamx_target_index_insert of the
   same points, alternating in one run on two identical indexes, median of 9 calls after 2; the first filtered call (it
   builds the occupancy table over the whole map) on its own.
2. filter: loamx_voxel_filter_dev alone on 24 k and 1 M device points.
3. drive: the size of the map over a canyon drive, with the filter and without."""
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
from loam_amd import build as B  # noqa: E402
from loam_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--drive-scans", type=int, default=257)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_bench.json"))
ap.add_argument("--only", default="")
args = ap.parse_args()
ctx = capi.Context(0)
out = dict(source_hash=B.source_hash())
EDGE_LEAF, PLANAR_LEAF = 0.2, 0.4


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


if args.only in ("", "insert"):
    H5, W5 = 128, 2048
    lidar5 = capi.LidarParams(H5, W5, 1.0, 120.0)
    maps_p, maps_e, k = [], [], 0
    while sum(len(m) for m in maps_p) < 1_000_000:  # (tools/extra_configs.py's map, features taken by the library)
        s = capi.synth_scan_host(1000 + k, 0, 0, H5, W5, 0.01)
        e, p = ctx.extract_features(s, lidar5)
        maps_p.append(s[p]), maps_e.append(s[e])
        k += 1
    map_p, map_e = np.concatenate(maps_p), np.concatenate(maps_e)
    scans = []
    for j in range(12):  # 1 + 2 + 9 scans from nearby poses (different noise seeds): every call brings new points
        s = capi.synth_scan_host(5000 + j, 0, 0, H5, W5, 0.01)
        e, p = ctx.extract_features(s, lidar5)
        scans.append((s[e], s[p]))
    plain, filt = ctx.target_index(map_e, map_p), ctx.target_index(map_e, map_p)
    # both indexes outgrow their exactly-sized buffers first (one rebuild each, as in tests/test_gpu_index_insert.py)
    ctx.target_index_insert(plain, *scans[0])
    ctx.target_index_insert(filt, *scans[0])
    t_first, added_first = timed(lambda: ctx.target_index_insert_filtered(filt, *scans[1], None, EDGE_LEAF, PLANAR_LEAF))
    t_plain_first, _ = timed(lambda: ctx.target_index_insert(plain, *scans[1]))
    t_plain, t_filt, added = [], [], []
    for j in range(2, 12):
        tp, _ = timed(lambda: ctx.target_index_insert(plain, *scans[j]))
        tf, a = timed(lambda: ctx.target_index_insert_filtered(filt, *scans[j], None, EDGE_LEAF, PLANAR_LEAF))
        if j >= 3:  # (the first round allocates the merge's twin buffers)
            t_plain.append(tp), t_filt.append(tf), added.append(a)
    # the filter's share: the same calls with everything rejected (the same scan again) stop after the one read-back
    t_reject = [timed(lambda: ctx.target_index_insert_filtered(filt, *scans[11], None, EDGE_LEAF, PLANAR_LEAF)) for _ in range(5)]
    assert all(a == (0, 0) for _, a in t_reject)
    out["insert_into_config5_map"] = dict(
        map_planar_points=int(len(map_p)), map_edge_points=int(len(map_e)), scan_edge=int(len(scans[2][0])), scan_planar=int(len(scans[2][1])),
        leaves=[EDGE_LEAF, PLANAR_LEAF], calls=len(t_plain),
        plain_insert_ms_median=round(statistics.median(t_plain), 3), filtered_insert_ms_median=round(statistics.median(t_filt), 3),
        plain_insert_ms=[round(t, 3) for t in t_plain], filtered_insert_ms=[round(t, 3) for t in t_filt],
        filtered_added=[list(a) for a in added], first_filtered_call_ms=round(t_first, 3), first_filtered_call_added=list(added_first),
        plain_call_next_to_it_ms=round(t_plain_first, 3), filtered_call_that_adds_nothing_ms_median=round(statistics.median(t for t, _ in t_reject), 3),
        sizes_after=dict(plain=ctx.target_index_size(plain), filtered=ctx.target_index_size(filt)),
        stats_after=dict(plain=ctx.target_index_stats(plain), filtered=ctx.target_index_stats(filt)))
    print(json.dumps(out["insert_into_config5_map"]), flush=True)
    ctx.target_index_destroy(plain), ctx.target_index_destroy(filt)

if args.only in ("", "filter"):
    rng = np.random.default_rng(1)
    res = {}
    for n, leaf in ((24_000, 0.4), (1_000_000, 0.1)):
        pts = rng.uniform(-1, 1, (n, 3)) * np.array([60.0, 60.0, 3.0])
        d_in, d_out, d_idx, d_n = ctx.alloc(pts.nbytes).upload(pts), ctx.alloc(pts.nbytes), ctx.alloc(4 * n), ctx.alloc(8)
        pose = np.array([0.0, 0.0, 0.01, 1.0, 0.5, 0.2, 0.0])
        pose[:4] /= np.linalg.norm(pose[:4])
        times = []
        for rep in range(12):
            ctx.synchronize()
            t0 = time.perf_counter()
            ctx.voxel_filter_dev(d_in.ptr, n, leaf, d_out.ptr, d_n.ptr, d_idx.ptr, pose)
            ctx.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        kept = int(d_n.download(np.uint32, 1)[0])
        med = statistics.median(times[2:])
        res["%d_points" % n] = dict(leaf=leaf, kept=kept, ms_median=round(med, 4), ms_min=round(min(times[2:]), 4), points_per_s=round(n / med * 1e3))
        for b in (d_in, d_out, d_idx, d_n):
            b.free()
    out["voxel_filter_dev"] = res
    print(json.dumps(res), flush=True)

if args.only in ("", "drive"):
    import outdoor_scenes as S
    H, W, n = 64, 1024, args.drive_scans
    lidar = capi.LidarParams(H, W, 1.0, 120.0)
    o0, yaw0 = S.sensor_origin("canyon", 3)
    idx_f = idx_u = None
    sizes = []
    t_f = t_u = 0.0
    for i in range(n):  # ground-truth poses: the map's size is the subject here, not the registration
        origin, yaw = o0 + 0.8 * i * np.array([np.cos(yaw0), np.sin(yaw0), 0.0]), yaw0 + 0.006 * i
        scan = S.scan_at("canyon", 0, origin, yaw, H, W, 0.01, noise_seed=1000 + i)
        e, p = ctx.extract_features(scan, lidar)
        pose = S.yaw_pose(yaw, origin)
        if idx_f is None:
            moved_e, moved_p = ctx.voxel_filter(scan[e], 0.0, pose)[0], ctx.voxel_filter(scan[p], 0.0, pose)[0]
            idx_f, idx_u = ctx.target_index(moved_e, moved_p), ctx.target_index(moved_e, moved_p)
        else:
            dt, _ = timed(lambda: ctx.target_index_insert_filtered(idx_f, scan[e], scan[p], pose, EDGE_LEAF, PLANAR_LEAF))
            t_f += dt
            dt, _ = timed(lambda: ctx.target_index_insert_filtered(idx_u, scan[e], scan[p], pose, 0.0, 0.0))
            t_u += dt
        if i in (0, 1, 2, 4, 8, 16, 32, 64, 128, 256) or i == n - 1:
            sizes.append(dict(scan=i, filtered=ctx.target_index_size(idx_f), unfiltered=ctx.target_index_size(idx_u)))
    out["canyon_drive"] = dict(scans=n, leaves=[EDGE_LEAF, PLANAR_LEAF], map_size=sizes, insert_ms_mean_filtered=round(t_f / max(n - 1, 1), 3),
                               insert_ms_mean_unfiltered=round(t_u / max(n - 1, 1), 3))
    print(json.dumps(out["canyon_drive"]), flush=True)

if not args.only:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
