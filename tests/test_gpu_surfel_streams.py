"""The stream contract of the surfel map's device entry points (include/loamx.h, "surfel map": the names without a suffix),
checked by the gated call of tests/stream_common.py on a caller's stream handed over with loamx_ctx_set_stream. Their C names
carry no "_dev", so the table of tests/test_gpu_streams.py does not list them; the rows are here. Every row is class "a": the
work stays in stream order AND the call returns without waiting on the host."""
import ctypes as C

import numpy as np
import pytest

import posegraph_common as PG
import stream_common as SC
import surfel_common as M

pytestmark = pytest.mark.gpu

SEED = {"A": 1, "B": 2}
OFFSETS = np.array([0, 3000, 6000], dtype=np.uint64)
OTHER_OFFSETS = np.array([0, 10, 20], dtype=np.uint64)
REC = M.SURFEL_DTYPE.itemsize


def sz(a):
    return SC.array_ptr(a, C.c_size_t)


def posed_clouds(which, dtype):
    rng = np.random.default_rng([SEED[which], 18])
    pts = rng.uniform(-8.0, 8.0, (6000, 3))
    pts[:, 2] *= 0.25
    poses = np.ascontiguousarray(np.stack([PG.rand_pose(rng, 0.2, 2.0) for _ in range(2)]))
    return {"points": np.ascontiguousarray(pts.astype(dtype)), "poses": poses}


class SurfelRow(SC.Case):
    """add -> emit on a fresh map; with `clear`: add -> clear -> add without poses -> emit; with `query`: add -> query of the
    first thousand of the call's own points (double rows only: a query takes doubles)"""
    CAPACITY, NQ = 6144, 1000
    klass = "a"

    def __init__(self, f32=False, clear=False, query=False):
        self.f32, self.clear, self.query = f32, clear, query
        self.add = "surfel_map_add_clouds" + ("_f32" if f32 else "")
        self.name = "surfel_map_add" + ("_f32" if f32 else "") + ("_clear_add" if clear else "") + ("_query" if query else "_emit")
        self.symbols = tuple("loamx_" + s for s in [self.add, "surfel_map_query" if query else "surfel_map_emit"] + (["surfel_map_clear"] if clear else []))
        if query:
            self.outputs = {"rec": (np.uint8, self.NQ * REC), "dist": (np.float64, self.NQ), "count": (np.uint32, self.NQ)}
        else:
            self.outputs = {"rec": (np.uint8, self.CAPACITY * REC), "xyz": (np.float64, self.CAPACITY * 3), "normal": (np.float64, self.CAPACITY * 3),
                            "n": (np.uint32, 2)}

    def __repr__(self):
        return self.name

    def inputs(self, which, ctx):
        return posed_clouds(which, np.float32 if self.f32 else np.float64)

    def fresh(self, ctx):
        return ctx.surfel_map(max_voxels=1 << 14)

    def call(self, run, m):
        p = run.p
        off = OFFSETS.copy()
        # (the query row adds without poses: its positions are the call's own points as they lie in the buffer)
        run.raw(self.add, m._handle(), p["points"], 3, sz(off), 2, None if self.query else p["poses"], host=[(off, OTHER_OFFSETS)])
        if self.clear:
            run.raw("surfel_map_clear", m._handle())
            off = OFFSETS.copy()
            run.raw(self.add, m._handle(), p["points"], 3, sz(off), 2, None, host=[(off, OTHER_OFFSETS)])
        if self.query:
            run.raw("surfel_map_query", m._handle(), p["points"], 3, self.NQ, 1, p["rec"], p["dist"], p["count"])
        else:
            run.raw("surfel_map_emit", m._handle(), 1, p["rec"], p["xyz"], p["normal"], self.CAPACITY, p["n"])

    def compared(self, out):
        """the number, and the entries below it (the header promises nothing beyond min(n, capacity))"""
        if self.query:
            return out
        k = min(int(out["n"][0]), self.CAPACITY)
        return {"rec": out["rec"][:k * REC], "xyz": out["xyz"][:k * 3], "normal": out["normal"][:k * 3], "n": out["n"][:1]}

    def check(self, got, A):
        if self.query:
            # every queried point lies in a voxel of its own map, but for those the map dropped (nearer than min_range)
            near = np.linalg.norm(A["points"][:self.NQ].astype(np.float64), axis=1) < 0.5
            assert (got["count"][~near] > 0).all() and (~near).sum() > 900 and np.abs(got["dist"]).max() > 0.0
        else:
            assert 1000 < got["n"][0] <= self.CAPACITY, got["n"]


CASES = [SurfelRow(), SurfelRow(f32=True), SurfelRow(clear=True), SurfelRow(query=True)]


def test_the_rows_are_the_four_the_handle_needs():
    assert [c.name for c in CASES] == ["surfel_map_add_emit", "surfel_map_add_f32_emit", "surfel_map_add_clear_add_emit", "surfel_map_add_query"]
    assert all(c.klass == "a" for c in CASES)
    covered = {s for c in CASES for s in c.symbols}
    assert covered == {"loamx_surfel_map_add_clouds", "loamx_surfel_map_add_clouds_f32", "loamx_surfel_map_emit", "loamx_surfel_map_query",
                       "loamx_surfel_map_clear"}


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_gated_call(case):
    SC.gated(case)
