#!/usr/bin/env python3
"""bench.py — scan-pair registrations per second on MI355X (BASELINE.json's metric).

One "step" = one pass of the whole hot path over one batch of synthetic 64x1024 scan pairs that is
already resident in HBM: extractFeatures(target scan) + extractFeatures(source scan) +
registerFeatures(source, target, identity) for every pair of the batch, through the C ABI
(loamx_register_scan_pairs_dev). Workload = BASELINE.json configs[2]/[3]: 1024 pairs per GPU
(weak scaling: every rank gets its own 1024 pairs, sharded by pair id, no data-path collective;
the only communication is the gather of the 64-byte result records: RCCL behind the C ABI,
loamx_gather_results_dev, inside the timed step).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--pairs P] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

`--gpus N` with N > 1 and no WORLD_SIZE in the environment: this process starts the N ranks itself
(`python -m torch.distributed.run` as a CHILD process, before torch or HIP are touched here) and exits
with the child's code.

A plain run sets up, warms up, times K steps and prints ONE JSON line on rank 0: metric, value, unit,
higher_is_better, dtype, ms_per_step (wall time of one timed step) and the configuration.
`--dump-outputs DIR` then also writes the result records of the last timed step (every pair of the step,
gathered over the ranks), as the caller of the path receives them: DIR/pose.npy (float64, pairs x 7:
qx qy qz qw tx ty tz), DIR/termination.npy and DIR/iterations.npy (float64, one per pair). The scans
are synthesised from --seed, so the same arguments give the same inputs on every run.

`--full` adds, after the timed steps, the objects below (--no-kernel-stats, --no-cpu-baseline, --no-streamed leave out the first three):
  roofline     — dominant kernel scope: algorithmic bytes per launch / average launch duration measured
                 with HIP events on the launch stream, vs 8 TB/s HBM peak; `compute` = vector-instruction
                 roofline of the (instruction-bound) k-NN kernel from the committed PMC pass
  cpu_baseline — the CPU oracle (oracle/, a port of the reference path) timed on this host's cores
                 on a bounded sample of the same pairs (rank 0, N=1 only): all threads + one thread
  extra        — streamed: the same pairs from PINNED HOST memory to host results (loamx_register_scan_pairs: chunked uploads on
                 a copy stream under the kernels), double and float scans: pairs/s and the PCIe rate reached, + the latency of
                 one pair from host buffers. Never `value`: the headline is device-resident
  results      — terminations and mean ICF iterations of the batch
  ranks        — (N > 1) what RCCL reported: communicator size, the gathered rank ids and devices
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8 TB/s HBM3E peak (6.3 TB/s achievable)
# vector-instruction issue peak: 256 CUs x 4 SIMDs x 2.4 GHz / 4 cycles per wave64 instruction = 614.4 G
# wave-instructions / s. MEASURED on this part (tools/probes/lds_unaligned.hip, profiles/r03_probe_lds_valu.txt): streams
# of independent v_med3_u32 / v_and_or_b32 / v_pk_fma_f32 / v_fma_f64 — the k-NN kernel's own mix — issue one
# instruction per 4.1-4.3 cycles per SIMD with 4-8 wavefronts resident (5.3-5.5 with one). The guide's "2 cycles
# (SIMD-32)" did not show for any of them, so round 2's figure (priced against 2 cycles) was half the real fraction.
VALU_CYCLES_PER_INST = 4
VALU_PEAK_GINST = 256 * 4 * 2.4 / VALU_CYCLES_PER_INST
SEED = 20240311
H, W = 64, 1024
SIGMA = 0.01
PMC_FILE = os.path.join(ROOT, "profiles", "r06_pmc.json")


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pairs", type=int, default=1024, help="scan pairs per GPU per step (weak scaling: the default)")
    ap.add_argument("--total-pairs", type=int, default=0,
                    help="fixed TOTAL pairs per step, sharded over the ranks by loamx_shard_range (strong scaling: BASELINE "
                         "configs[3] = 8192 over 1/2/4/8 GPUs); shards may be uneven (grouped ncclBroadcast path)")
    ap.add_argument("--cpu-sample", type=int, default=-1, help="pairs timed on the CPU oracle, all threads (default: ~3 s of wall time)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-kernel-stats", action="store_true", help="skip the extra timed-kernels pass (roofline / kernel table)")
    ap.add_argument("--input", choices=["f64", "f32"], default="f64",
                    help="scalar type of the resident scans: f64 (the headline workload) or f32 (SURVEY 8f4: sensor data as "
                         "floats, widened on load; arithmetic stays FP64)")
    ap.add_argument("--seed", type=int, default=SEED, help="seed of the synthetic scan pairs (default: the benchmark's)")
    ap.add_argument("--no-streamed", action="store_true",
                    help="skip the host-memory figure (extra.streamed: loamx_register_scan_pairs from pinned host scans, N = 1 only)")
    ap.add_argument("--streamed-pairs", type=int, default=512, help="pairs per call of the streamed figure (pinned host copy: 3.1 MB per pair)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure and check what the headline does not need: per-kernel event pass and "
                         "roofline, results summary, CPU baseline + parity, streamed figure, gather proof of the ranks")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the result records of the last timed step as DIR/pose.npy, termination.npy, iterations.npy (float64)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    return args


def dump_outputs(d, rec):
    """The records of the last timed step (RESULT_DTYPE, every pair of the step) as float64 arrays: 72 B per pair. The scans
    of a step are resident in HBM at 3.1 MB per pair, so 8 GPUs of 288 GB hold fewer than 750 k pairs: < 54 MB of output."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    np.save(os.path.join(d, "pose.npy"), np.ascontiguousarray(rec["pose"], dtype=np.float64))
    np.save(os.path.join(d, "termination.npy"), rec["termination"].astype(np.float64))
    np.save(os.path.join(d, "iterations.npy"), rec["iterations"].astype(np.float64))


def fan_out(args):
    """--gpus N without a launcher: start the N ranks under torch.distributed.run as a child process. Nothing in this
    process has imported torch or touched HIP yet, and this process never re-execs itself."""
    from loam_amd import build as B
    B.build()  # hipcc only (no GPU call): the ranks then find the library up to date instead of all building it at once
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


def source_hash():
    from loam_amd import build as B
    return B.source_hash()


def cgroup_cpu_quota():
    """CPUs this process may use at once according to its cgroup (cpu.max / cfs quota), or None if unlimited."""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if q == "max" else float(q) / float(per)
    except Exception:
        pass
    try:
        q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return q / per if q > 0 else None
    except Exception:
        return None


def cpu_baseline(scans, pairs, threads):
    """Times the oracle (extract x2 + register per pair) on `threads` host threads; returns (outputs, wall seconds)."""
    from concurrent.futures import ThreadPoolExecutor
    import oracle_lib as O
    O.build()
    O.lib()

    def one(pr):
        A, B = scans[2 * pr], scans[2 * pr + 1]
        ea, pa = O.extract_features(A, H, W, 1.0, 120.0)
        eb, pb = O.extract_features(B, H, W, 1.0, 120.0)
        pose, term, iters = O.register_features(B[eb], B[pb], A[ea], A[pa])
        return (ea, pa, eb, pb), pose, term, iters

    one(pairs[0])  # warm the caches / page in the library
    t0 = time.perf_counter()
    if threads == 1:
        out = [one(pr) for pr in pairs]
    else:
        with ThreadPoolExecutor(max_workers=threads) as ex:
            out = list(ex.map(one, pairs))
    return out, time.perf_counter() - t0


def streamed_figure(ctx, capi, xyz, n, lidar, fe, reg, f32_resident, dev_results):
    """Host scans in, host results out through loamx_register_scan_pairs: the first n pairs of the batch, pinned, as doubles
    and as floats. PCIe-bound by construction (3.1 MB per pair against ~10 us of kernels)."""
    import numpy as np
    import torch
    N = H * W
    out = {"entry_point": "loamx_register_scan_pairs / _f32 (chunks of 128 pairs, double-buffered hipMemcpyAsync on a copy stream under the kernels)",
           "pairs_per_call": n, "host_memory": "pinned (torch pin_memory)"}
    src = xyz[: n * 2 * N * 3]
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        if name == "f64" and f32_resident:
            continue  # (the resident batch was rounded to float: no double scans to stream)
        host = torch.empty(n * 2 * N * 3, dtype=dt, pin_memory=True)
        host.copy_(src.to(dt).cpu())
        arr = host.numpy()
        res = np.zeros(n, dtype=capi.RESULT_DTYPE)
        ctx.register_scan_pairs(arr, n, lidar, fe, reg, out=res)  # warm-up: staging buffers, workspace
        steps = 3
        t0 = time.perf_counter()
        for _ in range(steps):
            ctx.register_scan_pairs(arr, n, lidar, fe, reg, out=res)
        dt_s = (time.perf_counter() - t0) / steps
        entry = {"pairs_per_s": round(n / dt_s, 1), "ms_per_call": round(dt_s * 1e3, 3),
                 "pcie_GBs": round(arr.nbytes / dt_s / 1e9, 2), "bytes_per_pair": arr.nbytes // n}
        if name == "f64" and not f32_resident:
            entry["bit_identical_to_device_resident_results"] = bool(np.array_equal(res.view(np.uint8), dev_results[:n].view(np.uint8)))
        out[name] = entry
        if name == ("f32" if f32_resident else "f64"):  # one pair from host buffers: latency of the reference's own unit of use
            one = np.zeros(1, dtype=capi.RESULT_DTYPE)
            first = arr[: 2 * N * 3]
            for _ in range(5):
                ctx.register_scan_pairs(first, 1, lidar, fe, reg, out=one)
            K = 50
            t0 = time.perf_counter()
            for _ in range(K):
                ctx.register_scan_pairs(first, 1, lidar, fe, reg, out=one)
            out["one_pair_gpu_host_buffers_ms"] = round((time.perf_counter() - t0) / K * 1e3, 3)
        del host
    return out


def main():
    args = parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(fan_out(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")

    import numpy as np
    import torch
    import torch.distributed as dist

    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # LOAMX_BENCH_SHARE_GPU=1: rehearsal of the N>1 code path on a box with ONE GPU (all ranks on device 0; RCCL
    # refuses two ranks on one device, so the records are gathered through host memory with gloo). Never used by the
    # real multi-GPU run, which is one rank per GPU with the RCCL gather behind the C ABI.
    share_gpu = os.environ.get("LOAMX_BENCH_SHARE_GPU") == "1"
    n_dev = torch.cuda.device_count()  # (does not initialise the GPU)
    if n_dev < 1:
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    if world > 1 and not share_gpu and n_dev < world:
        raise SystemExit(f"bench.py --gpus {world}: only {n_dev} GPU(s) visible (one rank per GPU; LOAMX_BENCH_SHARE_GPU=1 "
                         "rehearses the N>1 path on one GPU)")
    dev_index = 0 if share_gpu else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        if share_gpu:
            dist.init_process_group(backend="gloo")
        else:
            dist.init_process_group(backend="nccl", device_id=dev)  # rendezvous + barriers (torch's "nccl" is RCCL)
    n_gpus = world

    from loam_amd import capi
    from loam_amd import distributed as D
    # the context keeps its own (non-blocking) stream: extraction, registration and the RCCL gather are all enqueued
    # on it, so the gather is ordered after the kernels that write the records by the stream itself
    ctx = capi.Context(dev_index)
    lidar = capi.LidarParams(H, W, 1.0, 120.0)  # reference README.md:45
    fe, reg = capi.FeatureExtractionParams(), capi.RegistrationParams()

    N = H * W
    strong = args.total_pairs > 0
    total_per_step = args.total_pairs if strong else world * args.pairs
    first_pair, P = capi.shard_range(total_per_step, world, rank)  # rank r owns pairs [first_pair, first_pair + P)
    if not strong:
        assert P == args.pairs
    if P == 0:
        raise SystemExit(f"bench.py: rank {rank} would own no pair of {total_per_step}")
    xyz = torch.empty(P * 2 * N * 3, dtype=torch.float64, device=dev)  # inputs resident in HBM
    results = torch.zeros(P * 64, dtype=torch.uint8, device=dev)
    all_results = torch.zeros(total_per_step * 64, dtype=torch.uint8, device=dev) if world > 1 else results
    torch.cuda.synchronize()
    ctx.synth_scan_pairs_dev(args.seed, first_pair, P, H, W, SIGMA, xyz.data_ptr())
    ctx.synchronize()
    f32 = args.input == "f32"
    if f32:  # the same scans rounded to float: half the resident bytes
        xyz = xyz.float()
        torch.cuda.synchronize()

    comm = None
    if world > 1 and not share_gpu:
        uid = [capi.comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(uid, src=0)
        comm = capi.Comm(ctx, uid[0], world, rank)

    def step():
        ctx.register_scan_pairs_dev(xyz.data_ptr(), P, lidar, fe, reg, results.data_ptr(), f32=f32)
        if comm is not None:  # the only collective: 64-byte result records, RCCL over xGMI on the context's stream
            comm.gather_results_dev(results.data_ptr(), P, total_per_step, all_results.data_ptr())
        elif world > 1:  # single-GPU rehearsal: through the host
            ctx.synchronize()
            all_results.copy_(D.gather_results(results.cpu(), total_per_step))

    def barrier():
        ctx.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if share_gpu else dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    res_all = res = None
    if args.full or args.dump_outputs:  # what the last timed step handed its caller: every rank's records, gathered
        res_all = all_results.cpu().numpy().view(capi.RESULT_DTYPE)
        res = res_all[first_pair:first_pair + P]
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, res_all)

    # ---- per-kernel pass: the same steps again with HIP events on the kernels (outside the headline timing: a
    # timed dispatch carries a completion signal, which costs ~2.5 % of the step) ------------------------------------
    stats, stat_steps = {}, 0
    if args.full and not args.no_kernel_stats:
        stat_steps = max(1, min(args.steps, 3))
        ctx.enable_kernel_timing(True)
        ctx.reset_kernel_stats()
        for _ in range(stat_steps):
            step()
        barrier()
        stats = ctx.kernel_stats()
        ctx.enable_kernel_timing(False)

    ranks = None
    if args.full and world > 1:
        # what the collective saw: every rank contributes one record {rank, device}; gathered through the same entry point
        proof = np.zeros(1, dtype=capi.RESULT_DTYPE)
        proof["termination"], proof["iterations"] = rank, dev_index
        own = bool(np.array_equal(res.view(np.uint8), results.cpu().numpy()))  # my block of the gathered array is my output
        if comm is not None:
            d_proof = torch.from_numpy(proof.view(np.uint8).copy()).to(dev)
            d_proof_all = torch.zeros(world * 64, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            comm.gather_results_dev(d_proof.data_ptr(), 1, world, d_proof_all.data_ptr())
            ctx.synchronize()
            got = d_proof_all.cpu().numpy().view(capi.RESULT_DTYPE)
            info = comm.info()
            ok = comm.barrier(0.0 if own else 1.0) == 0.0
            ranks = {"world_size": world, "rccl_comm_nranks": info["world_size"], "collective": "RCCL ncclAllGather behind the C ABI (loamx_gather_results_dev)",
                     "gathered_rank_ids": [int(x) for x in got["termination"]], "gathered_devices": [int(x) for x in got["iterations"]],
                     "records_gathered_per_step": total_per_step, "every_rank_holds_its_block": bool(ok)}
        else:
            got = D.gather_results(torch.from_numpy(proof.view(np.uint8).copy()), world).numpy().view(capi.RESULT_DTYPE)
            ranks = {"world_size": world, "rccl_comm_nranks": None, "collective": "gloo all_gather through host memory (LOAMX_BENCH_SHARE_GPU=1 "
                     "rehearsal: all ranks share device 0, which RCCL refuses)", "gathered_rank_ids": [int(x) for x in got["termination"]],
                     "gathered_devices": [int(x) for x in got["iterations"]], "records_gathered_per_step": total_per_step,
                     "every_rank_holds_its_block": own}

    total_pairs = total_per_step * args.steps
    value = total_pairs / elapsed

    if rank == 0:
        out = {
            "metric": "scan-pair registrations/sec (64x1024 Ouster)", "value": round(value, 2), "unit": "pairs/s",
            "n_gpus": n_gpus, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "strong" if strong else "weak",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": (f"batch of {total_per_step} independent 64x1024 scan pairs sharded over {n_gpus} GPU(s) (BASELINE configs[3]); "
                                    if strong else f"batch of {P} independent 64x1024 scan pairs per GPU (BASELINE configs[2]/[3]); ") +
                                   "step = extractFeatures x2 + registerFeatures per pair, inputs resident in HBM",
                       "pairs_per_gpu": P, "total_pairs_per_step": total_per_step, "scan": "64x1024", "sharding": "by pair id, no data-path collective",
                       "seed": args.seed, "range_noise_sigma_m": SIGMA, "input_scalar": args.input,
                       "arithmetic": "f64 (float input is widened on load)"},
        }
        if ranks:
            out["ranks"] = ranks
        # ---- roofline of the dominant kernel scope (and the per-kernel table) ----------------------------
        kern = {}
        for name, s in stats.items():
            if s["launches"] == 0:
                continue
            avg_ms = s["total_ms"] / s["launches"]
            kern[name] = dict(launches=s["launches"], total_ms=round(s["total_ms"], 4), avg_ms=round(avg_ms, 5),
                              algorithmic_bytes_per_launch=s["algorithmic_bytes"] / s["launches"])
        if "select_kernel" in kern:  # (loamx_ctx_get_kernel_stats prices the copies: the kernel counts its features)
            kern["select_kernel"]["algorithmic_bytes_note"] = "curvature words read + 2 x 24 B per feature copied (features counted by the kernel)"
        for name, k in kern.items():
            b = k["algorithmic_bytes_per_launch"]
            k["achieved_GBs"] = round(b / (k["avg_ms"] * 1e-3) / 1e9, 2) if b > 0 and k["avg_ms"] > 0 else None
            k["hbm_frac"] = round(k["achieved_GBs"] / HBM_PEAK_GBS, 4) if k["achieved_GBs"] else None
        if kern:
            top = {n: k for n, k in kern.items() if n != "knn_plane_kernel"}  # (a sub-scope of associate_kernel)
            dominant = max(top, key=lambda n: top[n]["total_ms"])
            dk = kern[dominant]
            # `scope` = the HIP-event scope the numbers below are measured over (one launch of every kernel of the association:
            # k-NN + fit, edge + plane, queue chain); `kernel` = the rocprofv3 kernel that dominates that scope and the step
            roofline = dict(kernel=dominant, scope=dominant, bound="hbm", achieved=dk["achieved_GBs"], peak=HBM_PEAK_GBS, unit="GB/s",
                            frac=dk["hbm_frac"], traffic=None,
                            avg_launch_ms=dk["avg_ms"], algorithmic_bytes_per_launch=dk["algorithmic_bytes_per_launch"],
                            share_of_kernel_time=round(dk["total_ms"] / sum(k["total_ms"] for k in top.values()), 4),
                            measured_over_steps=stat_steps)
            # The dominant kernel's live duration (HIP events around that launch alone: sub-scope knn_plane_kernel) and, from the
            # committed trace of the same sources, rocprofv3's own average and share of kernel time
            if dominant == "associate_kernel" and "knn_plane_kernel" in kern:
                roofline["kernel"] = "associate_knn_mixed_kernel<5, 5>"
                roofline["kernel_detail"] = {
                    "name": "associate_knn_mixed_kernel<5, 5>", "avg_us": round(kern["knn_plane_kernel"]["avg_ms"] * 1e3, 1),
                    "share": round(kern["knn_plane_kernel"]["total_ms"] / sum(k["total_ms"] for k in top.values()), 4),
                    "measured": "HIP events on the launch stream, this run"}
            # the HBM-bound kernels of the path (the ones north_star prices against the roofline), next to it
            roofline["hbm_bound_kernels"] = {n: kern[n]["hbm_frac"] for n in ("curvature_valid_kernel", "extract_fused_kernel", "sweep_kernel", "moment_kernel") if n in kern}
            # HBM traffic per launch of the dominant scope and the vector-instruction counts of the k-NN kernel come
            # from the committed rocprofv3 PMC passes of this same command; they are only valid for the kernels they
            # were measured on, so the file carries a hash of loam_amd/csrc and a mismatch nulls them
            try:
                pmc = json.load(open(PMC_FILE))
                h_now = source_hash()
                if pmc.get("source_sha256") != h_now:
                    roofline["traffic_note"] = f"{os.path.relpath(PMC_FILE, ROOT)} was profiled on other kernel sources ({pmc.get('source_sha256')} vs {h_now}): traffic not reported"
                elif pmc.get("bench_config", {}).get("pairs_per_gpu") == P:
                    tr = pmc.get("kernel_trace", {})
                    if tr and "kernel_detail" in roofline:
                        big = max(tr, key=lambda n: tr[n]["share"])
                        roofline["kernel_detail"].update({"rocprofv3_name": big, "rocprofv3_avg_us": tr[big]["avg_us"],
                                                                    "rocprofv3_share": tr[big]["share"],
                                                                    "rocprofv3_source": os.path.relpath(PMC_FILE, ROOT)})
                    # an event scope holds one dispatch of every kernel of that family (e.g. associate = kNN + fit,
                    # edge + plane): traffic per scope = sum of the per-dispatch averages
                    names = [k for k in pmc["kernels"] if k.startswith(dominant.replace("_kernel", ""))]
                    if names:
                        roofline["traffic"] = sum(pmc["kernels"][k]["traffic_bytes_per_dispatch"] for k in names)
                        roofline["traffic_source"] = f"{os.path.relpath(PMC_FILE, ROOT)} (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE, separate passes; sources {h_now})"
                    ctr = pmc.get("counters", {})
                    # (the plane round-1 k-NN kernel: on its own, or — every edge set small, k = 5 — one launch with the edge sets'
                    # brute-force search as its first workgroups)
                    knn = next((k for k in ctr if k.startswith("associate_knn_mixed_kernel") or k.startswith("associate_knn_kernel<true")), None)
                    if knn and "SQ_INSTS_VALU" in ctr[knn] and "knn_plane_kernel" in kern:
                        insts = ctr[knn]["SQ_INSTS_VALU"]  # wave-instructions per dispatch
                        ach = insts / (kern["knn_plane_kernel"]["avg_ms"] * 1e-3) / 1e9
                        comp = {"kernel": knn, "bound": "valu-issue", "achieved": round(ach, 1), "peak": VALU_PEAK_GINST,
                                "unit": "G wave-instructions/s", "frac": round(ach / VALU_PEAK_GINST, 4),
                                "valu_instructions_per_launch": insts, "avg_launch_ms": kern["knn_plane_kernel"]["avg_ms"]}
                        if "SQ_THREAD_CYCLES_VALU" in ctr[knn] and "SQ_ACTIVE_INST_VALU" in ctr[knn] and ctr[knn]["SQ_ACTIVE_INST_VALU"] > 0:
                            comp["active_lane_fraction"] = round(ctr[knn]["SQ_THREAD_CYCLES_VALU"] / (64.0 * ctr[knn]["SQ_ACTIVE_INST_VALU"]), 4)
                            comp["note"] = ("peak = one wave64 vector instruction per 4 cycles per SIMD, measured with the kernel's own "
                                            "instruction mix (profiles/r03_probe_lds_valu.txt: 4.1-4.3 cycles at 4-8 wavefronts per SIMD)")
                        if ctr[knn].get("TA_BUSY_avr") and ctr[knn].get("GRBM_GUI_ACTIVE"):
                            # second limiter of the same kernel: the texture addressers (per-lane 16-byte gathers of the
                            # candidate batches). TA_BUSY_avr = busy cycles averaged over the TAs, GRBM_GUI_ACTIVE is
                            # summed over the 8 XCDs
                            comp["texture_addresser_busy_frac"] = round(ctr[knn]["TA_BUSY_avr"] / (ctr[knn]["GRBM_GUI_ACTIVE"] / 8.0), 4)
                        roofline["compute"] = comp
            except Exception as e:  # no profile committed for this round yet
                roofline["traffic_note"] = f"no usable PMC file ({type(e).__name__})"
            out["roofline"] = roofline
            out["kernels"] = kern
        if args.full:
            out["results"] = {"converged": int((res["termination"] == 0).sum()), "max_iter": int((res["termination"] == 1).sum()),
                              "insufficient": int((res["termination"] == 2).sum()),
                              "mean_icf_iterations": round(float(res["iterations"].mean()), 3)}

        # ---- CPU baseline + parity spot check (outside the timed region) -----------------------------
        if args.full and n_gpus == 1 and not args.no_cpu_baseline:
            import oracle_lib as O
            affinity = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
            quota = cgroup_cpu_quota()  # the GPU box hands one GPU's share of the host: 16 of its 256 CPUs
            threads = max(1, min(affinity, int(quota + 0.5)) if quota else affinity)
            # ~40-50 ms of CPU per pair: 64 pairs per thread ~ 3 s of wall time; one thread: 96 pairs ~ 3.7 s
            n_sample = args.cpu_sample if args.cpu_sample > 0 else min(P, 64 * threads)
            n_single = min(P, 96)
            scans = xyz[: n_sample * 2 * N * 3].double().cpu().numpy().reshape(n_sample * 2, N, 3)
            cpu_out, dt = cpu_baseline(scans, list(range(n_sample)), threads)
            _, dt1 = cpu_baseline(scans, list(range(min(n_single, n_sample))), 1)
            out["cpu_baseline"] = {"value": round(n_sample / dt, 3), "unit": "pairs/s", "cores": threads, "kind": "port",
                                   "sample": f"first {n_sample} pairs of the GPU batch (same seeds), CPU oracle "
                                             f"extract x2 + register per pair, one pair per thread, {dt:.2f} s wall",
                                   "single_thread": {"value": round(min(n_single, n_sample) / dt1, 3), "unit": "pairs/s", "cores": 1,
                                                     "sample": f"first {min(n_single, n_sample)} pairs, one at a time, {dt1:.2f} s wall "
                                                               "(comparable to the reference's README.md:31: 3.5 ms x 2 + 13 ms per pair)"},
                                   "host_cpu_count": os.cpu_count(), "host_affinity": affinity, "cgroup_cpu_quota": quota}
            max_rot = max_trans = 0.0
            term_equal = True
            for pr, (_, pose, term, iters) in enumerate(cpu_out):
                d = O.pose_compose(O.pose_inverse(pose), res[pr]["pose"])
                max_rot = max(max_rot, O.quat_angular_distance(d[:4], [0, 0, 0, 1.0]))
                max_trans = max(max_trans, float(np.linalg.norm(d[4:])))
                term_equal &= (term == res[pr]["termination"] and iters == res[pr]["iterations"])
            # feature index sets of a few sample scans, GPU vs oracle
            idx_equal = True
            for s in range(min(8, 2 * n_sample)):
                e, p = ctx.extract_features(scans[s], lidar, fe)
                oe, op = cpu_out[s // 2][0][2 * (s % 2)], cpu_out[s // 2][0][2 * (s % 2) + 1]
                idx_equal &= bool(np.array_equal(e, oe) and np.array_equal(p, op))
            out["parity"] = {"pairs_checked": n_sample, "se3_max_rot_err_rad": max_rot, "se3_max_trans_err_m": max_trans,
                             "tolerance": 1e-5, "termination_and_iterations_equal": bool(term_equal),
                             "feature_index_sequences_equal": idx_equal}
        # ---- the streamed figure (outside the headline: SURVEY 8d prices inputs resident in HBM) -------------
        if args.full and n_gpus == 1 and not args.no_streamed:
            try:
                out["extra"] = {"streamed": streamed_figure(ctx, capi, xyz, min(P, max(1, args.streamed_pairs)), lidar, fe, reg, f32, res)}
            except Exception as e:  # (e.g. no room for the pinned copy on this host)
                out["extra"] = {"streamed": {"error": f"{type(e).__name__}: {e}"}}
        print(json.dumps(out), flush=True)

    if comm is not None:
        comm.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    ctx.close()


if __name__ == "__main__":
    main()
