"""The timing interface (include/loamx.h, "per-kernel timing"): loamx_ctx_enable_kernel_timing, _reset_kernel_stats and
_get_kernel_stats, from which bench.py --full builds its roofline object. Once on the context's private stream and once on a
caller's stream handed over with loamx_ctx_set_stream: the events are recorded on whichever the context runs on."""
import math

import numpy as np
import pytest

import test_gpu_streams as T
from loam_amd import capi

pytestmark = pytest.mark.gpu

SCOPES = ("curvature_valid_kernel", "select_kernel", "compact_kernel", "grid_build_kernel", "associate_kernel", "sweep_kernel", "lm_kernels",
          "moment_kernel", "knn_plane_kernel", "extract_fused_kernel", "information_kernel", "cloud_accumulate_kernel",
          "cloud_accumulate_plain_kernel", "cloud_list_kernels", "cloud_emit_kernels")


class Harness:
    """a context of its own, on its private stream or on a torch stream, with a bracket of two torch events around calls"""

    def __init__(self, caller_stream):
        import torch
        self.torch = torch
        self.ctx = capi.Context(0)
        self.s = torch.cuda.Stream() if caller_stream else None
        if self.s is not None:
            assert self.s.cuda_stream != 0
            self.ctx.set_stream(self.s.cuda_stream)
        self.bufs = []

    def upload(self, a):
        b = self.ctx.alloc(max(np.ascontiguousarray(a).nbytes, 8)).upload(a)
        self.bufs.append(b)
        return b

    def room(self, nbytes):
        b = self.ctx.alloc(max(nbytes, 8))
        self.bufs.append(b)
        return b

    def bracket(self, fn):
        """fn() between two torch events: on the caller's stream the events are recorded on it; on the private stream, which
        torch cannot name, they stand on torch's own stream with the context drained before each. -> ms"""
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.ctx.synchronize()
        e0.record(self.s) if self.s is not None else e0.record()
        if self.s is None:
            e0.synchronize()
        fn()
        if self.s is None:
            self.ctx.synchronize()
        e1.record(self.s) if self.s is not None else e1.record()
        e1.synchronize()
        self.ctx.synchronize()
        return e0.elapsed_time(e1)

    def close(self):
        self.ctx.synchronize()
        for b in self.bufs:
            b.free()
        self.ctx.close()


def check_times(stats, bracket_ms, where):
    assert tuple(stats) == SCOPES
    for name, s in stats.items():
        assert math.isfinite(s["total_ms"]) and s["total_ms"] >= 0.0, (where, name, s)
        assert math.isfinite(s["algorithmic_bytes"]) and s["algorithmic_bytes"] >= 0.0, (where, name, s)
        # scopes of one kind may overlap across the auxiliary streams: each launch is bounded by the bracket, not their sum
        assert s["total_ms"] <= s["launches"] * bracket_ms, (where, name, s, bracket_ms)
        if s["launches"] == 0:
            assert s["total_ms"] == 0.0, (where, name, s)


def all_zero(stats):
    return all(s["launches"] == 0 and s["total_ms"] == 0.0 for s in stats.values())


@pytest.mark.parametrize("caller_stream", (False, True), ids=("private_stream", "caller_stream"))
def test_registration_scopes(caller_stream):
    h = Harness(caller_stream)
    try:
        c = h.ctx
        xyz = h.upload(T.synth_scans("A", 4))
        res, info = h.room(2 * 64), h.room(2 * capi.INFORMATION_DTYPE.itemsize)
        li, fe, reg = T.lidar(), T.fe_params(), T.reg_params()

        def pairs(with_info=False):
            c.register_scan_pairs_dev(xyz.ptr, 2, li, fe, reg, res.ptr, d_info=info.ptr if with_info else None)
            c.synchronize()
            return res.download(capi.RESULT_DTYPE, 2).copy()

        # off is the default: nothing is counted
        off = pairs()
        assert all_zero(c.kernel_stats())
        assert (off["iterations"] > 0).all()
        # on: the same bytes, and the scopes of a scan-pair registration
        c.enable_kernel_timing(True)
        got = []
        ms = h.bracket(lambda: got.append(pairs()))
        assert np.array_equal(got[0].view(np.uint8), off.view(np.uint8)), "timing changed a result"
        st = c.kernel_stats()
        check_times(st, ms, "pairs")
        for name in ("grid_build_kernel", "associate_kernel", "sweep_kernel", "lm_kernels"):
            assert st[name]["launches"] > 0, (name, st[name])
        # the extraction: the fused kernel, or the separate ones. On the default route the selection writes the final arrays itself
        # (LOAMX_ROUTE_FUSED_COMPACT: compact_kernel is then only the conditional fallback inside the selection's scope), so the
        # compact scope counts exactly when the route says compact_kernel gathered; NO_FUSED_COMPACT below makes it count
        route = c.last_extract_route()
        separate = [st[n]["launches"] > 0 for n in ("curvature_valid_kernel", "select_kernel", "compact_kernel")]
        assert (st["compact_kernel"]["launches"] > 0) == ("COMPACT" in route) and ("COMPACT" in route) != ("FUSED_COMPACT" in route), (route, st)
        assert st["extract_fused_kernel"]["launches"] > 0 or all(separate) or (separate[0] and separate[1] and "FUSED_COMPACT" in route), (route, st)
        assert st["information_kernel"]["launches"] == 0
        assert st["knn_plane_kernel"]["launches"] <= st["associate_kernel"]["launches"]
        assert all(st[n]["launches"] == 0 for n in SCOPES if n.startswith("cloud_"))
        # an information pass counts in its own scope, and leaves the records as they were
        ms2 = h.bracket(lambda: got.append(pairs(with_info=True)))
        assert np.array_equal(got[1].view(np.uint8), off.view(np.uint8))
        st2 = c.kernel_stats()
        check_times(st2, max(ms, ms2), "pairs + info")  # (the totals hold both brackets' launches: each is bounded by the longer)
        assert st2["information_kernel"]["launches"] > 0
        assert all(st2[n]["launches"] >= st[n]["launches"] for n in SCOPES)
        # with the gather as a kernel of its own all three separate scopes count, and the records keep their bytes
        c.reset_kernel_stats()
        c.set_option("NO_FUSED_COMPACT", 1)
        ms3 = h.bracket(lambda: got.append(pairs()))
        c.set_option("NO_FUSED_COMPACT", 0)
        assert np.array_equal(got[2].view(np.uint8), off.view(np.uint8))
        st3 = c.kernel_stats()
        check_times(st3, ms3, "pairs, NO_FUSED_COMPACT")
        assert "COMPACT" in c.last_extract_route()
        assert all(st3[n]["launches"] > 0 for n in ("curvature_valid_kernel", "select_kernel", "compact_kernel")), st3
        # reset zeroes everything; off stops the counting
        c.reset_kernel_stats()
        assert all_zero(c.kernel_stats()) and all(s["algorithmic_bytes"] == 0.0 for s in c.kernel_stats().values())
        c.enable_kernel_timing(False)
        assert np.array_equal(pairs().view(np.uint8), off.view(np.uint8))
        assert all_zero(c.kernel_stats())
    finally:
        h.close()


@pytest.mark.parametrize("caller_stream", (False, True), ids=("private_stream", "caller_stream"))
def test_cloud_map_scopes(caller_stream):
    h = Harness(caller_stream)
    maps = []
    try:
        c = h.ctx
        clouds = T.posed_clouds("A", np.float64, 14)
        n = len(clouds["points"])
        d_pts, d_f32 = h.upload(clouds["points"]), h.upload(clouds["points"].astype(np.float32))
        d_poses = h.upload(clouds["poses"])
        cap = 6144
        d_xyz, d_n = h.room(cap * 24), h.room(8)
        m = c.cloud_map(max_voxels=1 << 14)
        maps.append(m)

        def emitted():
            m.emit_dev(d_xyz.ptr, cap, d_n.ptr)
            c.synchronize()
            k = int(d_n.download(np.uint32, 1)[0])
            return d_xyz.download(np.float64, 3 * min(k, cap)).copy()

        m.add_clouds_dev(d_pts.ptr, 3, T.OFFSETS, d_poses.ptr)
        off = emitted()
        assert all_zero(c.kernel_stats())
        c.enable_kernel_timing(True)
        # an add counts the accumulate and the list scope; the plain form counts nothing by default
        m.clear()
        ms = h.bracket(lambda: m.add_clouds_dev(d_pts.ptr, 3, T.OFFSETS, d_poses.ptr))
        st = c.kernel_stats()
        check_times(st, ms, "add")
        assert st["cloud_accumulate_kernel"]["launches"] > 0 and st["cloud_accumulate_plain_kernel"]["launches"] == 0
        assert st["cloud_accumulate_kernel"]["algorithmic_bytes"] == 24.0 * n  # (the header's figure, exactly)
        assert st["cloud_list_kernels"]["launches"] > 0 and st["cloud_emit_kernels"]["launches"] == 0
        # an emit counts its own scope, and timing changes no byte
        got = []
        ms2 = h.bracket(lambda: got.append(emitted()))
        assert np.array_equal(got[0].view(np.uint8), off.view(np.uint8))
        st = c.kernel_stats()
        check_times(st, max(ms, ms2), "add + emit")
        assert st["cloud_emit_kernels"]["launches"] > 0
        # float input: 12 bytes per point offered
        c.reset_kernel_stats()
        assert all_zero(c.kernel_stats())
        m.clear()
        ms = h.bracket(lambda: m.add_clouds_dev(d_f32.ptr, 3, T.OFFSETS, d_poses.ptr, f32=True))
        st = c.kernel_stats()
        check_times(st, ms, "add f32")
        assert st["cloud_accumulate_kernel"]["algorithmic_bytes"] == 12.0 * n
        # one claim per point: the other scope
        c.reset_kernel_stats()
        c.set_option("NO_CLOUDMAP_COMBINE", 1)
        m.clear()
        ms = h.bracket(lambda: m.add_clouds_dev(d_pts.ptr, 3, T.OFFSETS, d_poses.ptr))
        st = c.kernel_stats()
        check_times(st, ms, "add plain")
        assert st["cloud_accumulate_plain_kernel"]["launches"] > 0 and st["cloud_accumulate_kernel"]["launches"] == 0
        assert st["cloud_accumulate_plain_kernel"]["algorithmic_bytes"] == 24.0 * n
        assert np.array_equal(emitted().view(np.uint8), off.view(np.uint8))
        # off stops the counting
        c.reset_kernel_stats()
        c.enable_kernel_timing(False)
        m.clear()
        m.add_clouds_dev(d_pts.ptr, 3, T.OFFSETS, d_poses.ptr)
        emitted()
        assert all_zero(c.kernel_stats())
    finally:
        for m in maps:
            m.close()
        h.close()


@pytest.mark.parametrize("caller_stream", (False, True), ids=("private_stream", "caller_stream"))
def test_surfel_map_counts_in_no_cloud_scope(caller_stream):
    """the surfel map runs the cloud map's add loop and list kernels, but has no rows of its own: with timing on, an add and an emit
    of a surfel map leave all four cloud_* rows (and every other) at zero launches"""
    h = Harness(caller_stream)
    m = None
    try:
        c = h.ctx
        c.enable_kernel_timing(True)
        m = c.surfel_map(max_voxels=1 << 12)
        m.add_cloud(capi.synth_scan_host(1, 0, 0, 16, 256, 0.01))
        records, n = m.emit()
        assert n > 0 and len(records) == n and int(m.stats()["points_used"]) > 0
        st = c.kernel_stats()
        assert tuple(st) == SCOPES
        for name in ("cloud_accumulate_kernel", "cloud_accumulate_plain_kernel", "cloud_list_kernels", "cloud_emit_kernels"):
            assert st[name]["launches"] == 0, (name, st[name])
        assert all_zero(st)
    finally:
        if m is not None:
            m.close()
        h.close()
