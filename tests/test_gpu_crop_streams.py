"""The stream contract of the map window's entry points (include/loamx.h, "map window"), checked by the gated call of
tests/stream_common.py on a caller's stream handed over with loamx_ctx_set_stream. Their C names carry no "_dev", so the table of
tests/test_gpu_streams.py does not list them; the rows are here: cloud map add -> crop -> emit, surfel map add -> crop -> emit and
occupancy add -> crop -> query, all class "a": the work stays in stream order AND the call returns without waiting on the host.
A handle's FIRST crop allocates its staging and may wait on the allocator, so fresh() makes one crop of the new, empty map."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (loaded before libloamx: the gate's kernels and the library then share one HIP runtime, whichever test runs first)

import cloudmap_common as CM
import localize_common as L
import stream_common as SC
from loam_amd import capi

pytestmark = pytest.mark.gpu

N_SCANS, PER = 2, L.H * L.W
OFFSETS = np.arange(N_SCANS + 1, dtype=np.uint64) * PER
OTHER_OFFSETS = np.arange(N_SCANS + 1, dtype=np.uint64) * 10
LO, HI = np.array([-8.0, -8.0, -8.0]), np.array([8.0, 8.0, 8.0])
OTHER_LO, OTHER_HI = np.array([-0.5, -0.5, -0.5]), np.array([0.5, 0.5, 0.5])
NEW = ("loamx_cloud_map_crop", "loamx_surfel_map_crop", "loamx_occupancy_crop")


def sz(a):
    return SC.array_ptr(a, C.c_size_t)


def dp(a):
    return SC.array_ptr(a, C.c_double)


class CropRow(SC.Case):
    """add of two scans into a fresh map -> crop to 8 m around the second scan's pose (in device memory) -> a read-out"""
    klass = "a"
    CAPACITY = 4096
    NQ = 500
    KINDS = {
        "cloud_map": ("cloud_map_add_clouds_dev", "cloud_map_crop", "cloud_map_emit_dev",
                      {"xyz": (np.float64, CAPACITY * 3), "count": (np.uint32, CAPACITY), "first": (np.uint32, CAPACITY), "n": (np.uint32, 2)}),
        "surfel_map": ("surfel_map_add_clouds", "surfel_map_crop", "surfel_map_emit",
                       {"records": (np.uint8, CAPACITY * 128), "n": (np.uint32, 2)}),
        "occupancy": ("occupancy_add_clouds_dev", "occupancy_crop", "occupancy_query_dev",
                      {"q_counts": (np.uint32, 2 * NQ), "q_state": (np.uint8, NQ)}),
    }

    def __init__(self, kind):
        self.kind = kind
        self.add, self.crop, self.read, outputs = self.KINDS[kind]
        self.outputs = dict(outputs, counts=(np.uint32, 4))
        self.name = kind + "_add_crop_" + ("query" if kind == "occupancy" else "emit")
        self.symbols = tuple("loamx_" + s for s in (self.add, self.crop, self.read))

    def __repr__(self):
        return self.name

    def inputs(self, which, ctx):
        scans, poses = L.drive({"A": "lot", "B": "canyon"}[which])
        d = {"points": np.ascontiguousarray(scans[:N_SCANS].reshape(-1, 3)), "poses": np.ascontiguousarray(poses[:N_SCANS]),
             "centre": np.ascontiguousarray(poses[N_SCANS - 1])}
        if self.kind == "occupancy":  # queries along the beams of the second scan, inside the window and outside
            rng = np.random.default_rng(77)
            pick = rng.choice(PER, self.NQ, replace=False)
            d["queries"] = np.ascontiguousarray(CM.pose_act(poses[1], scans[1][pick] * rng.uniform(0.2, 1.0, (self.NQ, 1))))
        return d

    def fresh(self, ctx):
        if self.kind == "cloud_map":
            m = ctx.cloud_map(capi.CloudMapParams(0.5), 1 << 14)
        elif self.kind == "surfel_map":
            m = ctx.surfel_map(max_voxels=1 << 14)
        else:
            m = ctx.occupancy_map(capi.OccupancyParams(leaf=0.5), 1 << 18)
        m.crop_dev(LO, HI)  # the handle's allocation happens here, not inside the gated call
        ctx.synchronize()
        return m

    def call(self, run, m):
        p = run.p
        off = OFFSETS.copy()
        run.raw(self.add, m._handle(), p["points"], 3, sz(off), N_SCANS, p["poses"], host=[(off, OTHER_OFFSETS)])
        lo, hi = LO.copy(), HI.copy()
        run.raw(self.crop, m._handle(), p["centre"], dp(lo), dp(hi), p["counts"], host=[(lo, OTHER_LO), (hi, OTHER_HI)])
        if self.kind == "cloud_map":
            run.raw(self.read, m._handle(), 1, p["xyz"], p["count"], p["first"], self.CAPACITY, p["n"])
        elif self.kind == "surfel_map":
            run.raw(self.read, m._handle(), 1, p["records"], None, None, self.CAPACITY, p["n"])
        else:
            run.raw(self.read, m._handle(), p["queries"], 3, self.NQ, p["q_counts"], p["q_state"])

    def check(self, got, A):
        kept, removed, skipped, zero = (int(v) for v in got["counts"])
        assert kept > 100 and removed > 100 and skipped == 0 and zero == 0, got["counts"]
        if self.kind != "occupancy":
            assert int(got["n"][0]) == kept <= self.CAPACITY
        else:
            assert (got["q_state"] != 0).any() and (got["q_state"] == 0).any()  # (queries in the window and in what the crop removed)


CASES = [CropRow("cloud_map"), CropRow("surfel_map"), CropRow("occupancy")]


def test_the_rows_cover_the_three_new_entry_points():
    assert [c.name for c in CASES] == ["cloud_map_add_crop_emit", "surfel_map_add_crop_emit", "occupancy_add_crop_query"]
    assert all(c.klass == "a" for c in CASES)
    covered = {s for c in CASES for s in c.symbols}
    assert {s for s in covered if s.endswith("_crop")} == set(NEW) and all(sum(s in c.symbols for s in NEW) == 1 for c in CASES)
    lib = capi.load()
    assert covered <= set(capi.EXPORTS) and all(hasattr(lib, s) for s in covered)  # (the rows name entry points the library has)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_gated_call(case):
    SC.gated(case)
