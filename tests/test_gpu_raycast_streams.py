"""The stream contract of the ray cast's device forms (include/loamx.h, "occupancy ray casting"), checked by the gated call of
tests/stream_common.py on a caller's stream handed over with loamx_ctx_set_stream. Their C names carry no "_dev", so the table of
tests/test_gpu_streams.py does not list them; the row is here: occupancy add -> cast_rays -> render_scans, class "a": the work
stays in stream order AND the calls return without waiting on the host. A context's FIRST cast allocates its census words and may
wait on the allocator, so fresh() makes one cast on the new, empty map."""
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
LEAF, MAX_RANGE = 0.5, 40.0
N_RAYS, BEAMS = 300, (4, 70)
N_BEAMS = BEAMS[0] * BEAMS[1]
NEW = ("loamx_occupancy_cast_rays", "loamx_occupancy_render_scans")


def sz(a):
    return SC.array_ptr(a, C.c_size_t)


class RaycastRow(SC.Case):
    """add of two scans into a fresh map -> segments from the first pose cast through it -> the two scans rendered back"""
    name, klass = "occupancy_add_cast_rays_render_scans", "a"
    symbols = ("loamx_occupancy_add_clouds_dev",) + NEW
    outputs = {"records": (capi.RAY_RECORD_DTYPE, N_RAYS), "scans": (np.float64, N_SCANS * N_BEAMS * 3), "ranges": (np.float64, N_SCANS * N_BEAMS),
               "beam_records": (capi.RAY_RECORD_DTYPE, N_SCANS * N_BEAMS)}

    def __repr__(self):
        return self.name

    def inputs(self, which, ctx):
        scans, poses = L.drive({"A": "lot", "B": "canyon"}[which])
        poses = np.ascontiguousarray(poses[:N_SCANS])
        ends = np.ascontiguousarray(CM.pose_act(poses[0], scans[0][:N_RAYS].astype(np.float64)))
        origins = np.ascontiguousarray(np.broadcast_to(poses[0, 4:], ends.shape))
        return {"points": np.ascontiguousarray(scans[:N_SCANS].reshape(-1, 3)), "poses": poses, "origins": origins, "ends": ends,
                "dirs": capi.beam_directions(*BEAMS, capi.OrganizeParams(fov_bottom=np.radians(-12.0), fov_top=np.radians(6.0)))}

    def fresh(self, ctx):
        m = ctx.occupancy_map(capi.OccupancyParams(leaf=LEAF), 1 << 18)
        scratch = ctx.alloc(256)  # one segment: origin at 0, end at 64, its record at 128
        try:  # the context's allocation happens here, not inside the gated call
            scratch.upload(np.zeros(16))
            m.cast_rays_dev(scratch.ptr, scratch.ptr + 64, 3, 1, scratch.ptr + 128)
            ctx.synchronize()
        finally:
            scratch.free()
        return m

    def call(self, run, m):
        p = run.p
        off = OFFSETS.copy()
        run.raw("occupancy_add_clouds_dev", m._handle(), p["points"], 3, sz(off), N_SCANS, p["poses"], host=[(off, OTHER_OFFSETS)])
        st, other = capi.RaycastParams().struct(), capi.RaycastParams(unknown_stops=1, max_steps=1, hit_at=capi.RAY_AT_ENTER).struct()
        run.raw("occupancy_cast_rays", m._handle(), p["origins"], p["ends"], 3, N_RAYS, C.byref(st), p["records"], host=[(st, other)])
        st2 = capi.RaycastParams().struct()
        run.raw("occupancy_render_scans", m._handle(), p["dirs"], N_BEAMS, p["poses"], N_SCANS, C.c_double(MAX_RANGE), C.byref(st2), p["scans"],
                p["ranges"], p["beam_records"], host=[(st2, other)])

    def check(self, got, A):
        assert (got["records"]["status"] == capi.RAY_HIT).sum() > 100
        hit = got["beam_records"]["status"] == capi.RAY_HIT
        assert hit.sum() > 100 and (got["ranges"][hit] > 0).all() and not got["ranges"][~hit].any()


CASES = [RaycastRow()]


def test_the_row_covers_the_two_new_entry_points():
    assert [c.name for c in CASES] == ["occupancy_add_cast_rays_render_scans"] and CASES[0].klass == "a"
    covered = {s for c in CASES for s in c.symbols}
    assert set(NEW) <= covered
    lib = capi.load()
    assert covered <= set(capi.EXPORTS) and all(hasattr(lib, s) for s in covered)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_gated_call(case):
    SC.gated(case)
