"""The stream contract of the surfel localiser's device entry points (include/loamx.h, "surfel localisation": the names without a
suffix), checked by the gated call of tests/stream_common.py on a caller's stream handed over with loamx_ctx_set_stream. Their C
names carry no "_dev", so the table of tests/test_gpu_streams.py does not list them; the rows are here: add -> run and
add -> run_f32, both class "a": the work stays in stream order AND the call returns without waiting on the host."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (loaded before libloamx: the gate's kernels and the library then share one HIP runtime, whichever test runs first)

import localize_common as L
import stream_common as SC
from loam_amd import capi

pytestmark = pytest.mark.gpu

N_MAP, N_RUN, PER = 4, 2, L.H * L.W
MAP_OFFSETS = np.arange(N_MAP + 1, dtype=np.uint64) * PER
RUN_OFFSETS = np.arange(N_RUN + 1, dtype=np.uint64) * PER
OTHER_MAP_OFFSETS = np.arange(N_MAP + 1, dtype=np.uint64) * 10
OTHER_RUN_OFFSETS = np.arange(N_RUN + 1, dtype=np.uint64) * 10


def sz(a):
    return SC.array_ptr(a, C.c_size_t)


def drive_inputs(which, dtype):
    scans, poses = L.drive({"A": "lot", "B": "canyon"}[which])
    start = np.stack([L.displaced(poses[N_MAP + i], 0.1, 0.5, seed=i) for i in range(N_RUN)])
    return {"map_points": np.ascontiguousarray(scans[:N_MAP].reshape(-1, 3).astype(dtype)), "map_poses": np.ascontiguousarray(poses[:N_MAP]),
            "points": np.ascontiguousarray(scans[N_MAP:N_MAP + N_RUN].reshape(-1, 3).astype(dtype)), "start": np.ascontiguousarray(start)}


class LocalizeRow(SC.Case):
    """add of four scans into a fresh map -> run of two more from displaced poses"""
    klass = "a"

    def __init__(self, f32=False):
        self.f32 = f32
        self.add, self.run = "surfel_map_add_clouds" + ("_f32" if f32 else ""), "surfel_localizer_run" + ("_f32" if f32 else "")
        self.name = "surfel_add_localize" + ("_f32" if f32 else "")
        self.symbols = ("loamx_" + self.add, "loamx_" + self.run)
        self.outputs = {"poses": (np.float64, N_RUN * 7), "results": (np.uint8, N_RUN * 128), "info": (np.uint8, N_RUN * 696)}

    def __repr__(self):
        return self.name

    def inputs(self, which, ctx):
        return drive_inputs(which, np.float32 if self.f32 else np.float64)

    def fresh(self, ctx):
        m = ctx.surfel_map(max_voxels=1 << 15)
        return (m.localizer(N_RUN, N_RUN * PER), m)  # (dropped in this order: the localiser before its map)

    def call(self, run, state):
        loc, m = state
        p = run.p
        off = MAP_OFFSETS.copy()
        run.raw(self.add, m._handle(), p["map_points"], 3, sz(off), N_MAP, p["map_poses"], host=[(off, OTHER_MAP_OFFSETS)])
        off = RUN_OFFSETS.copy()
        st, other = capi.LocalizeParams().struct(), capi.LocalizeParams(max_iterations=1, neighborhood=1).struct()
        run.raw(self.run, loc._handle(), p["points"], 3, sz(off), N_RUN, p["start"], p["poses"], p["results"], p["info"], C.byref(st),
                host=[(off, OTHER_RUN_OFFSETS), (st, other)])

    def check(self, got, A):
        res = got["results"].view(L.RESULT_DTYPE)
        assert (res["termination"] == L.CONVERGED).all() and (res["n_rows"] > 1000).all(), res


CASES = [LocalizeRow(), LocalizeRow(f32=True)]


def test_the_rows_are_the_two_the_handle_needs():
    assert [c.name for c in CASES] == ["surfel_add_localize", "surfel_add_localize_f32"]
    assert all(c.klass == "a" for c in CASES)
    covered = {s for c in CASES for s in c.symbols}
    assert covered == {"loamx_surfel_map_add_clouds", "loamx_surfel_map_add_clouds_f32", "loamx_surfel_localizer_run", "loamx_surfel_localizer_run_f32"}
    lib = capi.load()
    assert covered <= set(capi.EXPORTS) and all(hasattr(lib, s) for s in covered)  # (the rows name entry points the library has)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_gated_call(case):
    SC.gated(case)
