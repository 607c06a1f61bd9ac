"""The stream contract of the occupancy distance field's device forms (include/loamx.h, "occupancy distance field"), checked by
the gated call of tests/stream_common.py on a caller's stream handed over with loamx_ctx_set_stream. Their C names carry no "_dev",
so the table of tests/test_gpu_streams.py does not list them; the row is here: occupancy add -> distance_box -> distance_slice,
class "a": the work stays in stream order AND the calls return without waiting on the host. A handle's FIRST distance call
allocates its staging and may wait on the allocator, so fresh() makes the two calls once on the new, empty map."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (loaded before libloamx: the gate's kernels and the library then share one HIP runtime, whichever test runs first)

import localize_common as L
import stream_common as SC
from loam_amd import capi

pytestmark = pytest.mark.gpu

N_SCANS, PER = 2, L.H * L.W
OFFSETS = np.arange(N_SCANS + 1, dtype=np.uint64) * PER
OTHER_OFFSETS = np.arange(N_SCANS + 1, dtype=np.uint64) * 10
LEAF, R = 0.5, 8
VMIN, DIMS = np.array([-24, -24, -2], dtype=np.int32), np.array([48, 48, 6], dtype=np.uint32)
OTHER_VMIN, OTHER_DIMS = np.array([500, 500, 500], dtype=np.int32), np.array([2, 2, 2], dtype=np.uint32)
N_BOX, N_SLICE = int(DIMS.prod()), int(DIMS[0] * DIMS[1])
NEW = ("loamx_occupancy_distance_box", "loamx_occupancy_distance_slice")


def sz(a):
    return SC.array_ptr(a, C.c_size_t)


class DistanceRow(SC.Case):
    """add of two scans into a fresh map -> the distance field of a box around the origin -> the field of its slice"""
    name, klass = "occupancy_add_distance_box_slice", "a"
    symbols = ("loamx_occupancy_add_clouds_dev",) + NEW
    outputs = {"box_d2": (np.uint16, N_BOX), "box_offset": (np.int16, 3 * N_BOX), "box_metres": (np.float32, N_BOX),
               "slice_d2": (np.uint16, N_SLICE), "slice_offset": (np.int16, 2 * N_SLICE), "slice_metres": (np.float32, N_SLICE)}

    def __repr__(self):
        return self.name

    def inputs(self, which, ctx):
        scans, poses = L.drive({"A": "lot", "B": "canyon"}[which])
        centre = poses[0, 4:]  # the box stands around the origin: the first pose goes there
        poses = np.ascontiguousarray(poses[:N_SCANS]).copy()
        poses[:, 4:] -= centre
        return {"points": np.ascontiguousarray(scans[:N_SCANS].reshape(-1, 3)), "poses": poses}

    def fresh(self, ctx):
        m = ctx.occupancy_map(capi.OccupancyParams(leaf=LEAF), 1 << 18)
        scratch = ctx.alloc(N_BOX * 2)
        try:  # the handle's allocation happens here, not inside the gated call
            m.distance_box_dev(VMIN, DIMS, capi.DistanceParams(R), scratch.ptr, 0, 0)
            m.distance_slice_dev(VMIN, DIMS, capi.DistanceParams(R), scratch.ptr, 0, 0)
            ctx.synchronize()
        finally:
            scratch.free()
        return m

    def call(self, run, m):
        p = run.p
        off = OFFSETS.copy()
        run.raw("occupancy_add_clouds_dev", m._handle(), p["points"], 3, sz(off), N_SCANS, p["poses"], host=[(off, OTHER_OFFSETS)])
        for name, pre in (("occupancy_distance_box", "box"), ("occupancy_distance_slice", "slice")):
            vmin, dims = VMIN.copy(), DIMS.copy()
            st, other = capi.DistanceParams(R).struct(), capi.DistanceParams(1, 1).struct()
            run.raw(name, m._handle(), SC.array_ptr(vmin, C.c_int32), SC.array_ptr(dims, C.c_uint32), C.byref(st), p[pre + "_d2"], p[pre + "_offset"],
                    p[pre + "_metres"], host=[(vmin, OTHER_VMIN), (dims, OTHER_DIMS), (st, other)])

    def check(self, got, A):
        for pre in ("box", "slice"):
            d2 = got[pre + "_d2"]
            assert (d2 == 0).sum() > 10 and ((d2 > 0) & (d2 < capi.DIST_FAR)).sum() > 200, pre
            assert np.isposinf(got[pre + "_metres"][d2 == capi.DIST_FAR]).all()


CASES = [DistanceRow()]


def test_the_row_covers_the_two_new_entry_points():
    assert [c.name for c in CASES] == ["occupancy_add_distance_box_slice"] and CASES[0].klass == "a"
    covered = {s for c in CASES for s in c.symbols}
    assert set(NEW) <= covered
    lib = capi.load()
    assert covered <= set(capi.EXPORTS) and all(hasattr(lib, s) for s in covered)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_gated_call(case):
    SC.gated(case)
