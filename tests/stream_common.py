"""The gated call: how tests/test_gpu_streams.py checks the stream contract of a "_dev" entry point (include/loamx.h: "run on the
context's stream and do not synchronise"; INTEGRATION.md section 6, "Streams").

A case (class Case) names its device inputs and outputs and enqueues one entry point, or a short chain, on a context of its own
that has adopted a caller's stream `s` through loamx_ctx_set_stream. Two valid inputs A and B of the same shapes give want_A and
want_B the plain way (synchronous upload, call, synchronise, download). Then, with B in the device inputs and 0xA5 in the device
outputs, everything goes onto `s` without a host synchronisation in between:

    torch.cuda._sleep (the gate) -> [class "a": the same call on B, in buffers and objects of its own] -> async H2D of A from pinned
    memory -> the entry point -> async D2H into pinned memory -> event

The call on B in front shares nothing with the one under test but the context: its stream and its workspaces. Whatever it leaves in
a workspace has to be reset, in stream order, by the call behind it; a reset that ran when it was enqueued (a memset on the null
stream) has by then been overwritten. Class "b" rows have none: their first host wait would drain the gate.

  ordering      the pinned outputs equal want_A by bytes. want_B instead: an input was read before the upload that `s` orders in
                front of the call (off-stream). 0xA5 left behind: the work was not joined into `s` before the download.
  no host wait  (class "a": the header says the call does not synchronise once warmed up) when the last enqueue has returned the
                event has not happened, and the host time since the gate's launch is under half the gate's measured duration. A
                gate too short for that fails the test; nothing skips.
  host args     every host struct and host array of the call is overwritten with other valid values as soon as the call has
                returned, that is, for class "a", while the gate still holds the stream.

Recorded on an MI355X (pytest -s prints them per case):
    the gate         10^7 cycles of torch.cuda._sleep = 4.16 ms, so 4.8 * 10^8 cycles for GATE_MS; measured 199.7 - 199.9 ms
    largest enqueue  warmed up and ungated: 0.65 ms in class "a" (loamx_pose_graph_optimize_dev, 3 iterations of 30 PCG steps),
                     1.3 ms for the chain of twelve calls; gate launch to last enqueue in class "a", the call on B in front
                     included: at most 1.2 ms. No case may exceed half the gate (asserted per case).
"""
import ctypes as C
import time

import numpy as np

from loam_amd import capi

GATE_MS = 200.0  # the target; the measured duration is what the assertions use
POISON = 0xA5
PROBE_CYCLES = 10_000_000

_gate = None  # (cycles, measured ms)


def torch_cuda():
    import torch
    return torch


def gate():
    """(cycles, ms): a torch.cuda._sleep of `cycles` takes `ms` (measured), as close to GATE_MS as one probe gets it"""
    global _gate
    if _gate is None:
        torch = torch_cuda()

        def timed(cycles):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        timed(PROBE_CYCLES)  # (the first launch of the kernel loads it)
        probe = timed(PROBE_CYCLES)
        assert probe > 0.0, "torch.cuda._sleep took no time"
        cycles = int(PROBE_CYCLES * GATE_MS / probe)
        ms = timed(cycles)
        print(f"\n[stream gate] {PROBE_CYCLES} cycles = {probe:.2f} ms -> {cycles} cycles = {ms:.1f} ms")
        assert 0.5 * GATE_MS <= ms <= 2.0 * GATE_MS, f"the gate measures {ms:.1f} ms, not about {GATE_MS} ms"
        _gate = (cycles, ms)
    return _gate


def bytes_of(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def same(a, b):
    a, b = bytes_of(a), bytes_of(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


def overwrite(obj, other):
    """other valid values over a host struct or array the library was handed"""
    if isinstance(obj, np.ndarray):
        assert obj.shape == np.shape(other)
        obj[...] = other
    else:
        assert C.sizeof(obj) == C.sizeof(other)
        C.memmove(C.addressof(obj), C.addressof(other), C.sizeof(obj))


def array_ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


class Case:
    """One row of the stream table. Subclasses give:
         symbols   the loamx_* entry points the case enqueues on the gated stream (tests/test_stream_table.py counts them)
         klass     "a": both assertions; "b": ordering only (the header says the call waits on the host)
         inputs(which, ctx) -> {name: array}   which in "A", "B": same shapes, other seeds, both valid
         outputs   {name: (dtype, count)}      device outputs, poisoned before every run; a name that is also an input is in-out
         fresh(ctx) -> state                   the objects the call works on, synchronised; made anew for every run
         call(run, state)                      enqueues; run.p[name] is a device address, run.raw(...) calls the library
         drop(state)
         compared(out) -> {name: array}        what of the downloaded outputs the header specifies (default: everything)
         check(got, A)                         further assertions on the gated outputs"""
    name, symbols, klass = "", (), "a"
    outputs = {}

    def inputs(self, which, ctx):
        return {}

    def fresh(self, ctx):
        return None

    def drop(self, state):
        if state is None:
            return
        for o in (state if isinstance(state, (tuple, list)) else (state,)):
            if hasattr(o, "close"):
                o.close()

    def call(self, run, state):
        raise NotImplementedError

    def compared(self, out):
        return out

    def check(self, got, A):
        """further assertions on the gated outputs (they equal want_A by then) and the inputs A"""


class Run:
    """what a case's call sees: the context, the device addresses and the library"""

    def __init__(self, ctx, p, step_sync=False):
        self.ctx, self.p, self.step_sync = ctx, p, step_sync

    def raw(self, name, *args, host=()):
        """loamx_<name>(ctx, *args); the (object, other valid values) pairs of `host` are overwritten as soon as it has returned"""
        rc = getattr(self.ctx.lib, "loamx_" + name)(self.ctx.h, *args)
        for obj, other in host:
            overwrite(obj, other)
        self.ctx._check(rc)
        if self.step_sync:
            self.ctx.synchronize()


class Buffers:
    """device tensors (bytes) for every input and output of a case, and pinned twins"""

    def __init__(self, case, shapes):
        torch = torch_cuda()
        self.torch = torch
        self.inputs = {k: np.ascontiguousarray(v).nbytes for k, v in shapes.items()}
        self.outputs = {k: np.dtype(dt).itemsize * int(n) for k, (dt, n) in case.outputs.items()}
        sizes = dict(self.outputs)
        sizes.update(self.inputs)
        for k in self.outputs:
            if k in self.inputs:
                assert self.outputs[k] == self.inputs[k], f"in-out buffer {k} has two sizes"
        self.dev = {k: torch.empty(max(n, 8), dtype=torch.uint8, device="cuda") for k, n in sizes.items()}
        self.pin_in = {k: torch.empty(max(n, 8), dtype=torch.uint8).pin_memory() for k, n in self.inputs.items()}
        self.pin_out = {k: torch.empty(max(n, 8), dtype=torch.uint8).pin_memory() for k, n in self.outputs.items()}
        self.p = {k: t.data_ptr() for k, t in self.dev.items()}
        self.dev2 = {k: torch.empty(max(n, 8), dtype=torch.uint8, device="cuda") for k, n in sizes.items()}  # the call in front
        self.p2 = {k: t.data_ptr() for k, t in self.dev2.items()}
        self.case = case

    def load(self, values, front=False):
        """synchronous: the inputs' bytes into the device inputs, poison into the pure outputs (front: of the call in front)"""
        torch = self.torch
        dev = self.dev2 if front else self.dev
        for k, t in dev.items():
            if k not in self.inputs:
                t.fill_(POISON)
        for k, v in values.items():
            b = bytes_of(v)
            dev[k][:len(b)].copy_(torch.from_numpy(b.copy()))
        torch.cuda.synchronize()

    def stage(self, values):
        for k, v in values.items():
            b = bytes_of(v)
            self.pin_in[k][:len(b)].copy_(torch_cuda().from_numpy(b.copy()))
        for t in self.pin_out.values():
            t.fill_(0)

    def read_sync(self):
        self.torch.cuda.synchronize()
        return self._typed({k: self.dev[k].cpu().numpy() for k in self.outputs})

    def read_pinned(self):
        return self._typed({k: self.pin_out[k].numpy().copy() for k in self.outputs})

    def _typed(self, raw):
        out = {}
        for k, (dt, n) in self.case.outputs.items():
            out[k] = raw[k][:np.dtype(dt).itemsize * int(n)].view(dt).copy()
        return out


def plain(case, ctx, bufs, values):
    """the plain way: synchronous upload, call (a synchronise behind every entry point of a chain), synchronise, download"""
    state = case.fresh(ctx)
    try:
        bufs.load(values)
        case.call(Run(ctx, bufs.p, step_sync=True), state)
        ctx.synchronize()
        return bufs.read_sync()
    finally:
        ctx.synchronize()
        case.drop(state)


def explain(case, got, want_a, want_b):
    """why the gated outputs differ from want_A, output by output"""
    g, a, b = case.compared(got), case.compared(want_a), case.compared(want_b)
    lines = []
    for k in a:
        if same(g[k], a[k]):
            continue
        gb, ab = bytes_of(g[k]), bytes_of(a[k])
        if same(g[k], b[k]):
            why = "equals want_B: an input was read off-stream, before the upload in front of the call"
        elif gb.shape == ab.shape and ((gb == POISON) & (ab != POISON)).any():
            why = f"{int(((gb == POISON) & (ab != POISON)).sum())} bytes of poison left: work was not joined into the stream before the download"
        else:
            why = f"{int((gb != ab).sum()) if gb.shape == ab.shape else '?'} bytes differ from want_A (and it is not want_B)"
        lines.append(f"{k}: {why}")
    return lines


def gated(case):
    """The protocol of this module's docstring on one case; raises AssertionError with the reason. Returns a dict of the measured
    times (ms): gate, enqueue (warmed up, ungated), host (gate launch to last enqueue)."""
    torch = torch_cuda()
    cycles, gate_ms = gate()
    ctx = capi.Context(0)
    s = torch.cuda.Stream()
    state = front = None
    try:
        assert s.cuda_stream != 0, "torch handed out the null stream"
        ctx.set_stream(s.cuda_stream)
        A, B = case.inputs("A", ctx), case.inputs("B", ctx)
        assert A.keys() == B.keys() and all(np.shape(A[k]) == np.shape(B[k]) and A[k].dtype == B[k].dtype for k in A), "A and B differ in shape"
        bufs = Buffers(case, A)
        want_a, want_b = plain(case, ctx, bufs, A), plain(case, ctx, bufs, B)
        ca, cb = case.compared(want_a), case.compared(want_b)
        for k in ca:
            assert not same(ca[k], cb[k]), f"{case.name}: output {k} is the same for A and B: the case cannot tell them apart"
        again = case.compared(plain(case, ctx, bufs, A))
        for k in ca:
            assert same(ca[k], again[k]), f"{case.name}: output {k} differs between two plain runs of A"

        # warm-up with the same sizes: every workspace has grown; its enqueue is what the gate has to cover
        state = case.fresh(ctx)
        bufs.load(A)
        t0 = time.perf_counter()
        case.call(Run(ctx, bufs.p), state)
        enqueue_ms = (time.perf_counter() - t0) * 1e3
        ctx.synchronize()
        case.drop(state)
        state = None

        # the gated run
        state = case.fresh(ctx)
        bufs.load(B)
        bufs.stage(A)
        if case.klass == "a":
            front = case.fresh(ctx)
            bufs.load(B, front=True)
        done = torch.cuda.Event()
        with torch.cuda.stream(s):
            t_gate = time.perf_counter()
            torch.cuda._sleep(cycles)
            if case.klass == "a":
                case.call(Run(ctx, bufs.p2), front)
            for k in bufs.inputs:
                bufs.dev[k].copy_(bufs.pin_in[k], non_blocking=True)
            case.call(Run(ctx, bufs.p), state)
            for k in bufs.outputs:
                bufs.pin_out[k].copy_(bufs.dev[k], non_blocking=True)
            done.record(s)
            host_ms = (time.perf_counter() - t_gate) * 1e3
            pending = not done.query()
        s.synchronize()
        got = bufs.read_pinned()
        print(f"\n[{case.name}] class {case.klass}: gate {gate_ms:.1f} ms, warmed-up enqueue {enqueue_ms:.2f} ms, gate launch to last enqueue {host_ms:.2f} ms")
        why = explain(case, got, want_a, want_b)
        assert not why, f"{case.name}: the gated run does not give want_A: " + "; ".join(why)
        case.check(got, A)
        if case.klass == "a":
            assert host_ms < 0.5 * gate_ms, (f"{case.name}: {host_ms:.1f} ms from the gate's launch to the last enqueue, the gate holds {gate_ms:.1f} ms: "
                                             f"the gate was too short for the no-host-wait check (warmed-up enqueue {enqueue_ms:.1f} ms), or the call waited for the stream")
            assert pending, f"{case.name}: the stream had drained when the last enqueue returned: the call waited on the host"
            assert enqueue_ms < 0.5 * gate_ms, f"{case.name}: the warmed-up enqueue takes {enqueue_ms:.1f} ms, more than half the gate"
        return dict(gate=gate_ms, enqueue=enqueue_ms, host=host_ms)
    finally:
        s.synchronize()
        try:
            ctx.synchronize()
        except capi.LoamxError:
            pass
        for st in (state, front):
            if st is not None:
                case.drop(st)
        ctx.close()
