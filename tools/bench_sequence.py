#!/usr/bin/env python3
"""Sequence entry points against the pair entry points on the SAME 256 pairs, and the de-skew kernel's bandwidth.

    python tools/bench_sequence.py                 # all steps -> profiles/sequence_bench.json
    python tools/bench_sequence.py --scans 33      # a shorter drive (rehearsal)

One drive through the ray-cast canyon (tests/outdoor_scenes.py: 257 scans of 64 x 1024, built once on the host, ~0.1 s of
CPU each) is registered through loamx_register_scan_sequence[_dev] and, as the duplicated layout [(scan p, scan p + 1)],
through loamx_register_scan_pairs[_dev]:
  resident   both device-resident forms, alternating, median ms per call over --steps calls after --warmup
  streamed   both host forms from pinned memory (torch pin_memory), the same way
  deskew     loamx_deskew_scans_dev over the 257 scans: GB/s against the 24 + 24 B per point it must move, next to
             curvature_valid_kernel's GB/s (33 B per point, the library's own per-kernel timing) on the same scans
Each step is a fresh child process under its own time limit; a step that fails ends the run. The results are checked
(sequence == pairs byte for byte) before anything is timed."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

H, W = 64, 1024
N = H * W
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E, specification
STEP_LIMIT_S = {"resident": 240, "streamed": 300, "deskew": 180}


def build_drive(n_scans):
    import numpy as np
    import outdoor_scenes as S
    o0, yaw0 = S.sensor_origin("canyon", 3)
    fwd = np.array([np.cos(yaw0), np.sin(yaw0), 0.0])
    out = np.empty((n_scans, N, 3))
    for i in range(n_scans):
        # (the street is 120 m long: the drive goes 24 m up the street and back again instead of leaving it; every step is
        # 0.8 m and 0.006 rad like the steps of the tests' sequences)
        k = i % 60
        k = k if k < 30 else 60 - k
        out[i] = S.scan_at("canyon", 0, o0 + 0.8 * k * fwd + np.array([0.0, 0.05 * np.sin(i), 0.0]), yaw0 + 0.006 * k, H, W, 0.01, noise_seed=1000 + i)
    return out


def median_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def alternate(fa, fb, steps, warmup):
    """median ms of two calls timed alternately (what one gains or loses to the box's other tenants, both do)"""
    for _ in range(warmup):
        fa(), fb()
    ta, tb = [], []
    for _ in range(steps):
        for f, ts in ((fa, ta), (fb, tb)):
            t0 = time.perf_counter()
            f()
            ts.append((time.perf_counter() - t0) * 1e3)
    return (statistics.median(ta), min(ta), max(ta)), (statistics.median(tb), min(tb), max(tb))


def step_resident(scans, args):
    import numpy as np
    from loam_amd import capi
    c = capi.Context(0)
    n, P = len(scans), len(scans) - 1
    lidar, fe, reg = capi.LidarParams(H, W, 1.0, 120.0), capi.FeatureExtractionParams(), capi.RegistrationParams()
    dup = np.ascontiguousarray(np.stack([scans[:-1], scans[1:]], axis=1))
    d_seq, d_dup = c.alloc(scans.nbytes).upload(scans), c.alloc(dup.nbytes).upload(dup)
    d_ra, d_rb = c.alloc(P * 64), c.alloc(P * 64)

    def run_seq():
        c.register_scan_sequence_dev(d_seq.ptr, n, lidar, fe, reg, d_ra.ptr)
        c.synchronize()

    def run_pairs():
        c.register_scan_pairs_dev(d_dup.ptr, P, lidar, fe, reg, d_rb.ptr)
        c.synchronize()

    run_seq(), run_pairs()
    ra, rb = d_ra.download(capi.RESULT_DTYPE, P), d_rb.download(capi.RESULT_DTYPE, P)
    same = bool(np.array_equal(ra.view(np.uint8), rb.view(np.uint8)))
    (ms_s, lo_s, hi_s), (ms_p, lo_p, hi_p) = alternate(run_seq, run_pairs, args.steps, args.warmup)
    return {"pairs": P, "records_identical": same, "converged": int((ra["termination"] == capi.CONVERGED).sum()),
            "sequence_ms": round(ms_s, 3), "sequence_ms_min_max": [round(lo_s, 3), round(hi_s, 3)],
            "pairs_ms": round(ms_p, 3), "pairs_ms_min_max": [round(lo_p, 3), round(hi_p, 3)],
            "sequence_ms_per_pair": round(ms_s / P, 5), "pairs_ms_per_pair": round(ms_p / P, 5),
            "sequence_over_pairs": round(ms_s / ms_p, 4)}


def step_streamed(scans, args):
    import numpy as np
    import torch
    from loam_amd import capi
    c = capi.Context(0)
    n, P = len(scans), len(scans) - 1
    lidar, fe, reg = capi.LidarParams(H, W, 1.0, 120.0), capi.FeatureExtractionParams(), capi.RegistrationParams()
    out = {"pairs": P, "host_memory": "pinned (torch pin_memory)", "chunk_pairs": c.get_option("STREAM_CHUNK_PAIRS") or 128}
    for name, dt, npdt in (("f64", torch.float64, np.float64), ("f32", torch.float32, np.float32)):
        h_seq = torch.empty(n * N * 3, dtype=dt, pin_memory=True)
        h_dup = torch.empty(P * 2 * N * 3, dtype=dt, pin_memory=True)
        a_seq, a_dup = h_seq.numpy(), h_dup.numpy()
        a_seq[:] = scans.astype(npdt).reshape(-1)
        a_dup.reshape(P, 2, N * 3)[:, 0] = a_seq.reshape(n, N * 3)[:-1]
        a_dup.reshape(P, 2, N * 3)[:, 1] = a_seq.reshape(n, N * 3)[1:]
        ra, rb = np.zeros(P, dtype=capi.RESULT_DTYPE), np.zeros(P, dtype=capi.RESULT_DTYPE)
        run_seq = lambda: c.register_scan_sequence(a_seq, n, lidar, fe, reg, out=ra)  # noqa: E731
        run_pairs = lambda: c.register_scan_pairs(a_dup, P, lidar, fe, reg, out=rb)  # noqa: E731
        run_seq(), run_pairs()
        same = bool(np.array_equal(ra.view(np.uint8), rb.view(np.uint8)))
        (ms_s, lo_s, hi_s), (ms_p, lo_p, hi_p) = alternate(run_seq, run_pairs, args.steps, args.warmup)
        out[name] = {"records_identical": same, "sequence_ms": round(ms_s, 3), "sequence_ms_min_max": [round(lo_s, 3), round(hi_s, 3)],
                     "pairs_ms": round(ms_p, 3), "pairs_ms_min_max": [round(lo_p, 3), round(hi_p, 3)],
                     "sequence_pairs_per_s": round(P / ms_s * 1e3, 1), "pairs_pairs_per_s": round(P / ms_p * 1e3, 1),
                     "sequence_bytes": int(a_seq.nbytes), "pairs_bytes": int(a_dup.nbytes),
                     "sequence_pcie_GBs": round(a_seq.nbytes / ms_s / 1e6, 2), "pairs_pcie_GBs": round(a_dup.nbytes / ms_p / 1e6, 2),
                     "speedup": round(ms_p / ms_s, 4), "byte_ratio": round(a_dup.nbytes / a_seq.nbytes, 4)}
        del h_seq, h_dup
    return out


def step_deskew(scans, args):
    import numpy as np
    from loam_amd import capi
    c = capi.Context(0)
    n = len(scans)
    lidar, fe = capi.LidarParams(H, W, 1.0, 120.0), capi.FeatureExtractionParams()
    rng = np.random.default_rng(5)
    motions = np.zeros((n, 7))
    ang = rng.uniform(0.002, 0.02, n)
    motions[:, 2], motions[:, 3] = np.sin(ang / 2), np.cos(ang / 2)
    motions[:, 4:] = [0.8, 0.0, 0.0] + rng.uniform(-0.05, 0.05, (n, 3))
    out = {"scans": n, "points": n * N}
    launches = 20
    for name, npdt, per_point in (("f64", np.float64, 48), ("f32", np.float32, 24)):
        data = np.ascontiguousarray(scans.astype(npdt))
        d_in, d_out, d_m = c.alloc(data.nbytes).upload(data), c.alloc(data.nbytes), c.alloc(motions.nbytes).upload(motions)

        def run():
            for _ in range(launches):
                c.deskew_scans_dev(d_in.ptr, n, lidar, d_m.ptr, d_out.ptr, 1.0, f32=npdt == np.float32)
            c.synchronize()

        ms, lo, hi = median_ms(run, args.steps, args.warmup)
        ms, lo, hi = ms / launches, lo / launches, hi / launches
        gbs = n * N * per_point / ms / 1e6
        out[name] = {"ms_per_launch": round(ms, 4), "ms_min_max": [round(lo, 4), round(hi, 4)], "bytes_per_point": per_point, "GBs": round(gbs, 1),
                     "fraction_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}
        if name == "f64":  # one scan alone: the launch is split over the lines to fill the chip
            def run_one():
                for _ in range(launches):
                    c.deskew_scans_dev(d_in.ptr, 1, lidar, d_m.ptr, d_out.ptr, 1.0)
                c.synchronize()
            one, _, _ = median_ms(run_one, args.steps, args.warmup)
            out["one_scan_us_per_launch"] = round(one / launches * 1e3, 2)
        for b in (d_in, d_out, d_m):
            b.free()
    # the curvature kernel on the same scans: the same access pattern (the library's own per-kernel timing)
    d_xyz = c.alloc(scans.nbytes).upload(scans)
    ecap, pcap = c.edge_capacity(lidar, fe), c.planar_capacity(lidar, fe)
    d_ne, d_np, d_ex, d_px = c.alloc(n * 4), c.alloc(n * 4), c.alloc(n * ecap * 24), c.alloc(n * pcap * 24)
    extract = lambda: c.extract_features_batch_dev(d_xyz.ptr, n, lidar, fe, 0, d_ne.ptr, d_ex.ptr, 0, d_np.ptr, d_px.ptr)  # noqa: E731
    for _ in range(args.warmup):
        extract()
    c.synchronize()
    c.enable_kernel_timing(True)
    c.reset_kernel_stats()
    for _ in range(args.steps):
        extract()
    st = c.kernel_stats()["curvature_valid_kernel"]
    c.enable_kernel_timing(False)
    if st["launches"] and st["total_ms"] > 0:
        gbs = st["algorithmic_bytes"] / st["total_ms"] / 1e6
        out["curvature_valid_kernel"] = {"launches": st["launches"], "ms_per_launch": round(st["total_ms"] / st["launches"], 4),
                                         "bytes_per_point": round(st["algorithmic_bytes"] / st["launches"] / (n * N), 2), "GBs": round(gbs, 1),
                                         "fraction_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}
        out["deskew_fraction_over_curvature_fraction"] = round(out["f64"]["GBs"] / gbs, 3)
    else:
        out["curvature_valid_kernel"] = "not measured (the separate curvature kernel did not run)"
    return out


STEPS = {"resident": step_resident, "streamed": step_streamed, "deskew": step_deskew}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=257)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=sorted(STEPS), action="append")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sequence_bench.json"))
    ap.add_argument("--step", choices=sorted(STEPS), help=argparse.SUPPRESS)   # child mode
    ap.add_argument("--data", help=argparse.SUPPRESS)
    args = ap.parse_args()
    import numpy as np
    if args.step:
        print("RESULT " + json.dumps(STEPS[args.step](np.load(args.data), args)), flush=True)
        return 0
    from loam_amd import build as B
    B.build()
    result = {"source_hash": B.source_hash(), "scan": [H, W], "scans": args.scans, "pairs": args.scans - 1, "steps": args.steps, "warmup": args.warmup,
              "timing": "host clock around calls that end in a stream synchronisation; median of `steps` calls, the two entry points alternating"}
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        path = os.path.join(tmp, "drive.npy")
        np.save(path, build_drive(args.scans))
        print("drive of %d scans built in %.1f s" % (args.scans, time.perf_counter() - t0), flush=True)
        for name in (args.only or ["resident", "streamed", "deskew"]):
            cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S[name]), sys.executable, os.path.abspath(__file__), "--step", name, "--data", path,
                   "--steps", str(args.steps), "--warmup", str(args.warmup)]
            run = subprocess.run(cmd, capture_output=True, text=True)
            lines = [ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
            if run.returncode != 0 or not lines:
                print(run.stdout[-2000:], run.stderr[-4000:], sep="\n")
                print("step %s failed with status %d: nothing further is started" % (name, run.returncode))
                return 1
            result[name] = json.loads(lines[-1][7:])
            print(name, json.dumps(result[name]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
