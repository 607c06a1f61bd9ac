"""The stream contract of every "_dev" entry point (include/loamx.h), checked by the gated call of
tests/stream_common.py on a caller's stream handed over with loamx_ctx_set_stream: one case per row of CASES, then the chain of
twelve calls behind one gate, a change of streams in mid flight, and the registration rows without the auxiliary streams.

Class "a" rows are the calls whose header comment says they do not synchronise once warmed up: both assertions. Class "b" rows
wait on the host by design (the registration family reads counts and live-pair words back; loamx_place_db_add_dev across a
growth): the ordering assertion only. tests/test_stream_table.py (CPU) holds every "_dev" symbol of the header against this table."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":  # (the child process of the last test: no conftest.py has put the repository on the path)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import map_common as MAP
import organize_common as ORG
import place_common as PLACE
import posegraph_common as PG
import segment_common as SEG
import stream_common as SC
import visibility_common as VIS
from loam_amd import capi

pytestmark = pytest.mark.gpu

H, W = 16, 256
N = H * W
# loamx_edge_capacity / loamx_planar_capacity at the default extraction parameters: per line and sector max + 1, but no more than
# the longest sector holds (the last of the six takes the remainder of the line)
CAP_E, CAP_P = H * 6 * min(11, W - 5 * (W // 6)), H * 6 * min(51, W - 5 * (W // 6))
SEED = {"A": 1, "B": 2}


def lidar(h=H, w=W):
    return capi.LidarParams(h, w, 1.0, 120.0)


def other_lidar():
    return capi.LidarParams(8, 64, 3.0, 40.0)


def fe_params():
    return capi.FeatureExtractionParams()


def other_fe():
    return capi.FeatureExtractionParams(2, 4, 3, 7, 50.0, 2.0, 0.25, 2.0)


def reg_params():
    r = capi.RegistrationParams()
    r.min_associations = 50
    return r


def other_reg():
    return capi.RegistrationParams(3, 0.5, 2, 5.0, 4, 1.0, 3, 0.2, 1, 1e-1, 1e-1, 5)


def rng_of(which, salt=0):
    return np.random.default_rng([SEED[which], salt])


def synth_scans(which, n, dtype=np.float64):
    """n scans of 16 x 256: the synthetic room's pairs (target, source), (target, source) ..."""
    scans = [capi.synth_scan_host(SEED[which], i // 2, i % 2, H, W, 0.01) for i in range(n)]
    return np.ascontiguousarray(np.stack(scans).astype(dtype))


def small_poses(rng, n, angle=0.05, extent=0.5):
    return np.ascontiguousarray(np.stack([PG.rand_pose(rng, angle, extent) for _ in range(n)]))


def sz(a):
    return SC.array_ptr(a, C.c_size_t)


class Row(SC.Case):
    def __init__(self, name, symbols, klass="a"):
        self.name, self.symbols, self.klass = name, tuple("loamx_" + s for s in symbols), klass

    def __repr__(self):
        return self.name


# ---- extraction ---------------------------------------------------------------------------------------------------------------------
class Extract(Row):
    outputs = {"edge_idx": (np.uint32, 2 * CAP_E), "n_edge": (np.uint32, 2), "edge_xyz": (np.float64, 2 * CAP_E * 3),
               "planar_idx": (np.uint32, 2 * CAP_P), "n_planar": (np.uint32, 2), "planar_xyz": (np.float64, 2 * CAP_P * 3)}

    def __init__(self, f32):
        self.f32 = f32
        Row.__init__(self, "extract_f32" if f32 else "extract", ["extract_features_batch_dev_f32" if f32 else "extract_features_batch_dev"])

    def inputs(self, which, ctx):
        return {"xyz": synth_scans(which, 2, np.float32 if self.f32 else np.float64)}

    def call(self, run, state):
        li, fe = lidar(), fe_params()
        assert run.ctx.edge_capacity(li, fe) == CAP_E and run.ctx.planar_capacity(li, fe) == CAP_P
        p = run.p
        run.raw("extract_features_batch_dev" + ("_f32" if self.f32 else ""), p["xyz"], 2, C.byref(li), C.byref(fe), p["edge_idx"], p["n_edge"],
                p["edge_xyz"], p["planar_idx"], p["n_planar"], p["planar_xyz"], host=[(li, other_lidar()), (fe, other_fe())])

    def compared(self, out):
        """the counts, and the entries below them (the header promises nothing beyond a scan's count)"""
        res = {"n_edge": out["n_edge"], "n_planar": out["n_planar"]}
        for kind, cap in (("edge", CAP_E), ("planar", CAP_P)):
            n = np.minimum(out["n_" + kind], cap)
            res[kind + "_idx"] = np.concatenate([out[kind + "_idx"][s * cap:s * cap + n[s]] for s in range(2)])
            res[kind + "_xyz"] = np.concatenate([out[kind + "_xyz"][s * cap * 3:(s * cap + n[s]) * 3] for s in range(2)])
        return res


# ---- registration family (class b: the counts and live-pair words come back to the host by design) --------------------------------
class FeatureBatch(Row):
    """loamx_register_features_batch_dev and loamx_registration_information_batch_dev on 2 pairs of extracted feature sets"""
    outputs = {"results": (capi.RESULT_DTYPE, 2), "info": (capi.INFORMATION_DTYPE, 2)}
    SETS = ("src_edge", "src_planar", "tgt_edge", "tgt_planar")

    def __init__(self):
        Row.__init__(self, "feature_batch", ["register_features_batch_dev", "registration_information_batch_dev"], "b")

    def inputs(self, which, ctx):
        scans = synth_scans(which, 4)
        out = {k: np.zeros((2, CAP_E if "edge" in k else CAP_P, 3)) for k in self.SETS}
        out.update({"n_" + k: np.zeros(2, dtype=np.uint32) for k in self.SETS})
        for pair in range(2):
            for role, scan in (("tgt", scans[2 * pair]), ("src", scans[2 * pair + 1])):
                e, p = ctx.extract_features(scan, lidar())
                for kind, idx in (("edge", e), ("planar", p)):
                    out[f"{role}_{kind}"][pair, :len(idx)] = scan[idx]
                    out[f"n_{role}_{kind}"][pair] = len(idx)
        return out

    def call(self, run, state):
        p = run.p
        for fn, out in (("register_features_batch_dev", "results"), ("registration_information_batch_dev", "info")):
            reg = reg_params()
            run.raw(fn, 2, p["src_edge"], p["n_src_edge"], p["src_planar"], p["n_src_planar"], p["tgt_edge"], p["n_tgt_edge"], p["tgt_planar"],
                    p["n_tgt_planar"], CAP_E, CAP_P, None, C.byref(reg), p[out], host=[(reg, other_reg())])


class ScanPairs(Row):
    def __init__(self, f32, info):
        self.f32, self.info = f32, info
        fn = "register_scan_pairs" + ("_info" if info else "") + "_dev" + ("_f32" if f32 else "")
        self.fn = fn
        self.outputs = {"results": (capi.RESULT_DTYPE, 2)}
        if info:
            self.outputs["info"] = (capi.INFORMATION_DTYPE, 2)
        Row.__init__(self, fn[len("register_"):], [fn], "b")

    def inputs(self, which, ctx):
        return {"xyz": synth_scans(which, 4, np.float32 if self.f32 else np.float64)}

    def call(self, run, state):
        li, fe, reg = lidar(), fe_params(), reg_params()
        tail = (run.p["info"],) if self.info else ()
        run.raw(self.fn, run.p["xyz"], 2, C.byref(li), C.byref(fe), C.byref(reg), run.p["results"], *tail,
                host=[(li, other_lidar()), (fe, other_fe()), (reg, other_reg())])


class ScanSequence(Row):
    def __init__(self, f32, info):
        self.f32, self.info = f32, info
        fn = "register_scan_sequence" + ("_info" if info else "") + "_dev" + ("_f32" if f32 else "")
        self.fn = fn
        self.outputs = {"results": (capi.RESULT_DTYPE, 3)}
        if info:
            self.outputs["info"] = (capi.INFORMATION_DTYPE, 3)
        Row.__init__(self, fn[len("register_"):], [fn], "b")

    def inputs(self, which, ctx):
        return {"xyz": synth_scans(which, 4, np.float32 if self.f32 else np.float64), "init": small_poses(rng_of(which, 1), 3, 0.01, 0.05)}

    def call(self, run, state):
        li, fe, reg = lidar(), fe_params(), reg_params()
        tail = (run.p["info"],) if self.info else ()
        run.raw(self.fn, run.p["xyz"], 4, C.byref(li), C.byref(fe), C.byref(reg), run.p["init"], run.p["results"], *tail,
                host=[(li, other_lidar()), (fe, other_fe()), (reg, other_reg())])


REGISTRATION_ROWS = [FeatureBatch()] + [ScanPairs(f32, info) for info in (False, True) for f32 in (False, True)] + \
    [ScanSequence(f32, info) for info in (False, True) for f32 in (False, True)]


# ---- trajectory and de-skew ------------------------------------------------------------------------------------------------------
def result_records(rng, n):
    rec = np.zeros(n, dtype=capi.RESULT_DTYPE)
    rec["pose"] = small_poses(rng, n, 0.1, 1.0)
    rec["termination"], rec["iterations"] = rng.integers(0, 3, n), rng.integers(1, 10, n)
    return rec


class Compose(Row):
    def __init__(self, n):
        self.n = n
        self.outputs = {"trajectory": (np.float64, (n + 1) * 7)}
        Row.__init__(self, f"compose_trajectory_{n}", ["compose_trajectory_dev"])

    def inputs(self, which, ctx):
        return {"results": result_records(rng_of(which, 2), self.n)}

    def call(self, run, state):
        origin = PG.rand_pose(np.random.default_rng(3), 1.0, 5.0)
        run.raw("compose_trajectory_dev", run.p["results"], self.n, SC.array_ptr(origin, C.c_double), run.p["trajectory"],
                host=[(origin, PG.rand_pose(np.random.default_rng(4), 1.0, 5.0))])


class Deskew(Row):
    def __init__(self, f32):
        self.f32 = f32
        self.outputs = {"out": (np.float32 if f32 else np.float64, 4 * N * 3)}
        Row.__init__(self, "deskew_f32" if f32 else "deskew", ["deskew_scans_dev_f32" if f32 else "deskew_scans_dev"])

    def inputs(self, which, ctx):
        return {"xyz": synth_scans(which, 4, np.float32 if self.f32 else np.float64), "motion": small_poses(rng_of(which, 5), 4)}

    def call(self, run, state):
        li = lidar()
        run.raw("deskew_scans_dev" + ("_f32" if self.f32 else ""), run.p["xyz"], 4, C.byref(li), run.p["motion"], 0.5, run.p["out"],
                host=[(li, other_lidar())])


# ---- unordered clouds, voxel filter ----------------------------------------------------------------------------------------------
OFFSETS = np.array([0, 3000, 6000], dtype=np.uint64)
OTHER_OFFSETS = np.array([0, 10, 20], dtype=np.uint64)


class Organize(Row):
    OH, OW = 16, 128

    def __init__(self, f32):
        self.f32 = f32
        cells = 2 * self.OH * self.OW
        self.outputs = {"scans": (np.float32 if f32 else np.float64, cells * 3), "src_idx": (np.uint32, cells), "stats": (np.uint32, 8)}
        Row.__init__(self, "organize_f32" if f32 else "organize", ["organize_clouds_dev_f32" if f32 else "organize_clouds_dev"])

    def inputs(self, which, ctx):
        return {"points": ORG.random_cloud(rng_of(which, 6), 6000).astype(np.float32 if self.f32 else np.float64)}

    def fresh(self, ctx):
        return ctx.scan_layout(lidar(self.OH, self.OW))

    def call(self, run, layout):
        off = OFFSETS.copy()
        run.raw("organize_clouds_dev" + ("_f32" if self.f32 else ""), layout._handle(), run.p["points"], 3, None, sz(off), 2, run.p["scans"],
                run.p["src_idx"], run.p["stats"], host=[(off, OTHER_OFFSETS)])


class VoxelFilter(Row):
    NP = 1025
    outputs = {"xyz_out": (np.float64, NP * 3), "src_idx": (np.uint32, NP), "n_out": (np.uint32, 2)}

    def __init__(self):
        Row.__init__(self, "voxel_filter", ["voxel_filter_dev"])

    def inputs(self, which, ctx):
        return {"xyz": MAP.surface_points(rng_of(which, 7), self.NP)}

    def call(self, run, state):
        pose = MAP.small_pose(np.random.default_rng(8))
        run.raw("voxel_filter_dev", run.p["xyz"], self.NP, SC.array_ptr(pose, C.c_double), 0.2, run.p["xyz_out"], run.p["src_idx"], run.p["n_out"],
                host=[(pose, MAP.small_pose(np.random.default_rng(9)))])

    def compared(self, out):
        n = min(int(out["n_out"][0]), self.NP)  # (entries past the count are unspecified)
        return {"n_out": out["n_out"][:1], "xyz_out": out["xyz_out"][:3 * n], "src_idx": out["src_idx"][:n]}


# ---- place recognition -----------------------------------------------------------------------------------------------------------
R_, S_, K_ = 20, 60, 5


def place_db_70(ctx):
    db = ctx.place_db(capi.PlaceParams(n_rings=R_, n_sectors=S_))
    db.add(PLACE.random_descriptors(np.random.default_rng(10), 70, R_, S_))  # (synchronises)
    return db


class PlaceDescriptors(Row):
    outputs = {"desc": (np.uint16, 2 * R_ * S_)}

    def __init__(self, f32):
        self.f32 = f32
        Row.__init__(self, "place_descriptors_f32" if f32 else "place_descriptors", ["place_descriptors_dev_f32" if f32 else "place_descriptors_dev"])

    def inputs(self, which, ctx):
        return {"points": PLACE.random_cloud(rng_of(which, 11), 6000).astype(np.float32 if self.f32 else np.float64)}

    def fresh(self, ctx):
        return ctx.place_db(capi.PlaceParams(n_rings=R_, n_sectors=S_))

    def call(self, run, db):
        off = OFFSETS.copy()
        run.raw("place_descriptors_dev" + ("_f32" if self.f32 else ""), db._handle(), run.p["points"], 3, sz(off), 2, run.p["desc"], host=[(off, OTHER_OFFSETS)])


class PlaceSearch(Row):
    """loamx_place_search_dev alone (n_add == 0), or behind loamx_place_db_add_dev of the queries' own descriptors: inside the
    capacity of the database's first allocation (256 entries) or across its growth (70 + 200 entries: the header's "unless the
    database has to grow", class b)"""

    def __init__(self, n_add):
        self.n_add = n_add
        self.n_desc = max(n_add, 3)
        self.outputs = {"matches": (capi.PLACE_MATCH_DTYPE, 3 * K_)}
        if n_add == 0:
            Row.__init__(self, "place_search", ["place_search_dev"])
        else:
            grows = 70 + n_add > 256
            Row.__init__(self, "place_add_growth_then_search" if grows else "place_add_then_search", ["place_db_add_dev", "place_search_dev"],
                         "b" if grows else "a")

    def inputs(self, which, ctx):
        return {"desc": PLACE.random_descriptors(rng_of(which, 12), self.n_desc, R_, S_)}

    fresh = staticmethod(place_db_70)

    def call(self, run, db):
        total = 70 + self.n_add
        if self.n_add:
            first = C.c_uint32(0xFFFFFFFF)
            run.raw("place_db_add_dev", db._handle(), run.p["desc"], self.n_add, C.byref(first))
            assert first.value == 70
        id_end = np.array([total, total - 1, 40], dtype=np.uint32)
        run.raw("place_search_dev", db._handle(), run.p["desc"], 3, id_end.ctypes.data, K_, run.p["matches"],
                host=[(id_end, np.array([1, 2, 3], dtype=np.uint32))])


# ---- pose graph -------------------------------------------------------------------------------------------------------------------
def pgo_struct(**kw):
    d = dict(max_iterations=3, max_pcg_iterations=30)
    d.update(kw)
    return capi.PgoParams(**d).struct()


class PgoOptimize(Row):
    """chain_graph(40, 3, closed=True); with `bad` one edge of A (two of B) has a == b: the summary says BAD_INPUT and the poses
    stay A's"""
    NPOSES = 40

    def __init__(self, bad):
        self.bad = bad
        self.outputs = {"poses": (np.float64, self.NPOSES * 7), "summary": (capi.PGO_SUMMARY_DTYPE, 1)}
        Row.__init__(self, "pose_graph_optimize_bad_edge" if bad else "pose_graph_optimize", ["pose_graph_optimize_dev"])

    def inputs(self, which, ctx):
        poses, edges, _ = PG.chain_graph(self.NPOSES, 3, 20 + SEED[which], closed=True)
        edges = np.ascontiguousarray(edges.astype(capi.PGO_EDGE_DTYPE))
        if self.bad:
            for k in range(SEED[which]):
                edges["b"][5 + k] = edges["a"][5 + k]
        return {"poses": np.ascontiguousarray(poses), "edges": edges}

    def call(self, run, state):
        self.n_edges = self.NPOSES - 1 + 1 + 3
        st = pgo_struct()
        run.raw("pose_graph_optimize_dev", run.p["poses"], self.NPOSES, None, run.p["edges"], self.n_edges, C.byref(st), run.p["summary"],
                host=[(st, pgo_struct(max_iterations=1, max_pcg_iterations=2, initial_lambda=10.0))])

    def check(self, got, A):
        s = got["summary"][0]
        if self.bad:
            assert s["termination"] == capi.PGO_BAD_INPUT and s["n_bad_edges"] == 1, s
            assert SC.same(got["poses"], A["poses"]), "a refused solve changed the poses"
        else:
            assert s["termination"] != capi.PGO_BAD_INPUT and s["iterations"] >= 1, s
            assert not SC.same(got["poses"], A["poses"])


def information_records(rng, n):
    rec = np.zeros(n, dtype=capi.INFORMATION_DTYPE)
    rec["information"] = np.stack([PG.rand_information(rng) for _ in range(n)])
    rec["eigenvalues"] = rng.uniform(1.0, 2.0, (n, 6))
    return rec


class PgoEdges(Row):
    """loamx_pose_graph_edges_from_results_dev alone, or (solve) followed by the solve of the graph it made: the odometry of a ring
    of 40 poses as result records, the poses dead-reckoned and then disturbed, so that the solve has something to do"""
    NPOSES = 40

    def __init__(self, solve):
        self.solve = solve
        n = self.NPOSES - 1
        self.outputs = {"edges": (capi.PGO_EDGE_DTYPE, n)}
        if solve:
            self.outputs.update({"poses": (np.float64, self.NPOSES * 7), "summary": (capi.PGO_SUMMARY_DTYPE, 1)})
            Row.__init__(self, "pose_graph_edges_then_optimize", ["pose_graph_edges_from_results_dev", "pose_graph_optimize_dev"])
        else:
            Row.__init__(self, "pose_graph_edges", ["pose_graph_edges_from_results_dev"])

    def inputs(self, which, ctx):
        rng = rng_of(which, 13)
        poses, edges, _ = PG.chain_graph(self.NPOSES, 0, 30 + SEED[which])
        res = np.zeros(self.NPOSES - 1, dtype=capi.RESULT_DTYPE)
        res["pose"], res["iterations"] = edges["a_T_b"], 3
        out = {"results": res, "info": information_records(rng, self.NPOSES - 1)}
        if self.solve:
            moved = PG.retract(poses, np.concatenate([0.01 * rng.normal(size=(self.NPOSES, 3)), 0.1 * rng.normal(size=(self.NPOSES, 3))], axis=1))
            moved[0] = poses[0]
            out["poses"] = np.ascontiguousarray(moved)
        return out

    def call(self, run, state):
        n = self.NPOSES - 1
        run.raw("pose_graph_edges_from_results_dev", run.p["results"], run.p["info"], n, 0, run.p["edges"])
        if self.solve:
            st = pgo_struct()
            run.raw("pose_graph_optimize_dev", run.p["poses"], self.NPOSES, None, run.p["edges"], n, C.byref(st), run.p["summary"],
                    host=[(st, pgo_struct(max_iterations=1, max_pcg_iterations=2))])


# ---- cloud map and occupancy map -----------------------------------------------------------------------------------------------
def posed_clouds(which, dtype, salt):
    rng = rng_of(which, salt)
    pts = rng.uniform(-8.0, 8.0, (6000, 3))
    pts[:, 2] *= 0.25
    return {"points": np.ascontiguousarray(pts.astype(dtype)), "poses": small_poses(rng, 2, 0.2, 2.0)}


class CloudMapRow(Row):
    """add -> emit on a fresh map; with `clear`: add -> clear -> add without poses -> emit"""
    CAPACITY = 6144
    outputs = {"xyz": (np.float64, CAPACITY * 3), "count": (np.uint32, CAPACITY), "first": (np.uint32, CAPACITY), "n": (np.uint32, 2)}

    def __init__(self, f32, clear=False):
        self.f32, self.clear = f32, clear
        add = "cloud_map_add_clouds_dev" + ("_f32" if f32 else "")
        self.add = add
        Row.__init__(self, "cloud_map_add" + ("_f32" if f32 else "") + ("_clear_add" if clear else "") + "_emit",
                     [add, "cloud_map_emit_dev"] + (["cloud_map_clear"] if clear else []))

    def inputs(self, which, ctx):
        return posed_clouds(which, np.float32 if self.f32 else np.float64, 14)

    def fresh(self, ctx):
        return ctx.cloud_map(max_voxels=1 << 14)

    def call(self, run, m):
        p = run.p
        off = OFFSETS.copy()
        run.raw(self.add, m._handle(), p["points"], 3, sz(off), 2, p["poses"], host=[(off, OTHER_OFFSETS)])
        if self.clear:
            run.raw("cloud_map_clear", m._handle())
            off = OFFSETS.copy()
            run.raw(self.add, m._handle(), p["points"], 3, sz(off), 2, None, host=[(off, OTHER_OFFSETS)])
        run.raw("cloud_map_emit_dev", m._handle(), 1, p["xyz"], p["count"], p["first"], self.CAPACITY, p["n"])

    def check(self, got, A):
        assert 1000 < got["n"][0] <= self.CAPACITY, got["n"]


class OccupancyRow(Row):
    """add -> query, box, slice on a fresh map; with `clear`: add -> clear -> add without poses -> query, box, slice"""
    NQ = 500
    VMIN, DIMS = np.array([-20, -20, -5], dtype=np.int32), np.array([40, 40, 10], dtype=np.uint32)
    OTHER_VMIN, OTHER_DIMS = np.array([0, 0, 0], dtype=np.int32), np.array([2, 2, 2], dtype=np.uint32)
    NBOX = 40 * 40 * 10
    outputs = {"q_counts": (np.uint32, 2 * NQ), "q_state": (np.uint8, NQ), "box_counts": (np.uint32, 2 * NBOX), "box_state": (np.uint8, NBOX),
               "grid": (np.uint8, 40 * 40)}

    def __init__(self, f32, clear=False):
        self.f32, self.clear = f32, clear
        add = "occupancy_add_clouds_dev" + ("_f32" if f32 else "")
        self.add = add
        Row.__init__(self, "occupancy_add" + ("_f32" if f32 else "") + ("_clear_add" if clear else "") + "_query_box_slice",
                     [add, "occupancy_query_dev", "occupancy_box_dev", "occupancy_slice_dev"] + (["occupancy_clear"] if clear else []))

    def inputs(self, which, ctx):
        d = posed_clouds(which, np.float32 if self.f32 else np.float64, 15)
        d["queries"] = rng_of(which, 16).uniform(-6.0, 6.0, (self.NQ, 3)) * np.array([1.0, 1.0, 0.25])
        return d

    def fresh(self, ctx):
        return ctx.occupancy_map(max_voxels=1 << 18)

    def call(self, run, m):
        p = run.p
        off = OFFSETS.copy()
        run.raw(self.add, m._handle(), p["points"], 3, sz(off), 2, p["poses"], host=[(off, OTHER_OFFSETS)])
        if self.clear:
            run.raw("occupancy_clear", m._handle())
            off = OFFSETS.copy()
            run.raw(self.add, m._handle(), p["points"], 3, sz(off), 2, None, host=[(off, OTHER_OFFSETS)])
        run.raw("occupancy_query_dev", m._handle(), p["queries"], 3, self.NQ, p["q_counts"], p["q_state"])
        for fn, outs in (("occupancy_box_dev", (p["box_counts"], p["box_state"])), ("occupancy_slice_dev", (p["grid"],))):
            vmin, dims = self.VMIN.copy(), self.DIMS.copy()
            run.raw(fn, m._handle(), SC.array_ptr(vmin, C.c_int32), SC.array_ptr(dims, C.c_uint32), *outs,
                    host=[(vmin, self.OTHER_VMIN), (dims, self.OTHER_DIMS)])

    def check(self, got, A):
        assert len(np.unique(got["box_state"])) == 3 and len(np.unique(got["grid"])) >= 2, "the box does not show all three states"


# ---- segmentation and map cleaning ----------------------------------------------------------------------------------------------
class Segment(Row):
    SH, SW, MAXC = 21, 300, 32

    def __init__(self, f32):
        self.f32 = f32
        cells = 2 * self.SH * self.SW
        self.outputs = {"classes": (np.uint8, cells), "labels": (np.uint32, cells), "sizes": (np.uint32, cells),
                        "filtered": (np.float32 if f32 else np.float64, cells * 3), "clusters": (capi.SEGMENT_CLUSTER_DTYPE, 2 * self.MAXC),
                        "stats": (np.uint32, 16)}
        Row.__init__(self, "segment_f32" if f32 else "segment", ["segment_scans_dev_f32" if f32 else "segment_scans_dev"])

    def inputs(self, which, ctx):
        five = SEG.five_scans(self.SH, self.SW)
        return {"scans": np.ascontiguousarray(five[[0, 1] if which == "A" else [4, 3]].astype(np.float32 if self.f32 else np.float64))}

    def call(self, run, state):
        p = run.p
        li, st = lidar(self.SH, self.SW), capi.SegmentParams().struct()
        run.raw("segment_scans_dev" + ("_f32" if self.f32 else ""), p["scans"], 2, C.byref(li), C.byref(st), p["classes"], p["labels"], p["sizes"],
                p["filtered"], p["clusters"], self.MAXC, p["stats"],
                host=[(li, other_lidar()), (st, capi.SegmentParams(ground_angle=0.5, segment_angle=0.3, min_cluster_points=2, drop_ground=1).struct())])


class Visibility(Row):
    """votes (written, or added to the votes the buffer holds) -> filter: 2 000 points against 2 scans of 16 x 256"""
    NP = 2000

    def __init__(self, f32, accumulate):
        self.f32, self.accumulate = f32, accumulate
        self.outputs = {"votes": (capi.VISIBILITY_VOTES_DTYPE, self.NP), "dynamic": (np.uint8, self.NP), "static_xyz": (np.float64, self.NP * 3),
                        "static_idx": (np.uint32, self.NP), "n_static": (np.uint32, 2)}
        Row.__init__(self, "visibility_votes" + ("_f32" if f32 else "") + ("_accumulate" if accumulate else "") + "_then_filter",
                     ["visibility_votes_dev" + ("_f32" if f32 else ""), "visibility_filter_dev"])

    def inputs(self, which, ctx):
        rng = rng_of(which, 17)
        scans = np.stack([VIS.shell_scan(rng, H, W, holes=False) for _ in range(2)]).astype(np.float32 if self.f32 else np.float64)
        d = {"points": VIS.cloud(rng, self.NP), "scans": np.ascontiguousarray(scans), "poses": small_poses(rng, 2, 0.1, 1.0)}
        if self.accumulate:
            d["votes"] = rng.integers(0, 4, (self.NP, 4)).astype(np.uint32).view(capi.VISIBILITY_VOTES_DTYPE).reshape(-1)
        return d

    def fresh(self, ctx):
        return ctx.scan_layout(lidar())

    def call(self, run, layout):
        p = run.p
        kw = dict(min_through=1, through_ratio=0.5)
        st = capi.VisibilityParams(**kw).struct()
        other = capi.VisibilityParams(min_range=5.0, max_range=10.0, margin=2.0, window_lines=0, window_cols=0, min_through=9).struct()
        run.raw("visibility_votes_dev" + ("_f32" if self.f32 else ""), layout._handle(), p["points"], 3, self.NP, p["scans"], 2, p["poses"], C.byref(st),
                1 if self.accumulate else 0, p["votes"], host=[(st, other)])
        st = capi.VisibilityParams(**kw).struct()
        run.raw("visibility_filter_dev", p["votes"], self.NP, C.byref(st), p["points"], 3, p["dynamic"], p["static_xyz"], p["static_idx"], self.NP,
                p["n_static"], host=[(st, other)])

    def check(self, got, A):
        assert 0 < got["n_static"][0] < self.NP, "the filter keeps all points or none"


CASES = [Extract(False), Extract(True)] + REGISTRATION_ROWS + [Compose(3), Compose(65), Deskew(False), Deskew(True), Organize(False), Organize(True),
                                                               VoxelFilter(), PlaceDescriptors(False), PlaceDescriptors(True), PlaceSearch(0),
                                                               PlaceSearch(3), PlaceSearch(200), PgoEdges(False), PgoOptimize(False), PgoOptimize(True),
                                                               PgoEdges(True), CloudMapRow(False), CloudMapRow(True), CloudMapRow(False, clear=True),
                                                               OccupancyRow(False), OccupancyRow(True), OccupancyRow(False, clear=True),
                                                               Segment(False), Segment(True)] + \
    [Visibility(f32, acc) for f32 in (False, True) for acc in (False, True)]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_gated_call(case):
    SC.gated(case)


# ---- the chain: twelve calls behind one gate ---------------------------------------------------------------------------------------
class Chain(Row):
    """organise -> de-skew -> sequence with information -> compose -> edges -> optimise -> cloud-map add -> emit -> occupancy add ->
    query -> votes -> filter on 4 clouds at 16 x 256, every step reading what the one before wrote. The plain runs synchronise after
    every step (Run.raw does under step_sync), the gated run once at the end. Class b: the sequence registration waits on the host."""
    NS, CAPACITY = 4, 8192
    outputs = {"scans": (np.float64, NS * N * 3), "deskewed": (np.float64, NS * N * 3), "results": (capi.RESULT_DTYPE, NS - 1),
               "info": (capi.INFORMATION_DTYPE, NS - 1), "trajectory": (np.float64, NS * 7), "edges": (capi.PGO_EDGE_DTYPE, NS - 1),
               "summary": (capi.PGO_SUMMARY_DTYPE, 1), "map_xyz": (np.float64, CAPACITY * 3), "map_n": (np.uint32, 2),
               "q_counts": (np.uint32, 2 * CAPACITY), "q_state": (np.uint8, CAPACITY), "votes": (capi.VISIBILITY_VOTES_DTYPE, CAPACITY),
               "dynamic": (np.uint8, CAPACITY), "n_static": (np.uint32, 2)}
    SYMBOLS = ["organize_clouds_dev", "deskew_scans_dev", "register_scan_sequence_info_dev", "compose_trajectory_dev",
               "pose_graph_edges_from_results_dev", "pose_graph_optimize_dev", "cloud_map_add_clouds_dev", "cloud_map_emit_dev",
               "occupancy_add_clouds_dev", "occupancy_query_dev", "visibility_votes_dev", "visibility_filter_dev"]

    def __init__(self):
        Row.__init__(self, "chain", self.SYMBOLS, "b")

    def inputs(self, which, ctx):
        rng = rng_of(which, 18)
        scans = synth_scans(which, self.NS)
        clouds = np.ascontiguousarray(np.concatenate([s[rng.permutation(N)] for s in scans]))
        # the emit's room is an input (zeros) so that the query and the votes behind it never read poison past the voxel count
        return {"points": clouds, "motion": small_poses(rng, self.NS, 0.01, 0.05), "map_xyz": np.zeros(self.CAPACITY * 3)}

    def fresh(self, ctx):
        return [ctx.scan_layout(lidar()), ctx.cloud_map(max_voxels=1 << 16), ctx.occupancy_map(max_voxels=1 << 18)]

    def call(self, run, state):
        layout, cmap, omap = state
        p, ns = run.p, self.NS
        off = (np.arange(ns + 1) * N).astype(np.uint64)
        run.raw("organize_clouds_dev", layout._handle(), p["points"], 3, None, sz(off), ns, p["scans"], None, None, host=[(off, off // 2)])
        li = lidar()
        run.raw("deskew_scans_dev", p["scans"], ns, C.byref(li), p["motion"], 1.0, p["deskewed"], host=[(li, other_lidar())])
        li, fe, reg = lidar(), fe_params(), reg_params()
        run.raw("register_scan_sequence_info_dev", p["deskewed"], ns, C.byref(li), C.byref(fe), C.byref(reg), None, p["results"], p["info"],
                host=[(li, other_lidar()), (fe, other_fe()), (reg, other_reg())])
        run.raw("compose_trajectory_dev", p["results"], ns - 1, None, p["trajectory"])
        run.raw("pose_graph_edges_from_results_dev", p["results"], p["info"], ns - 1, 0, p["edges"])
        st = pgo_struct()
        run.raw("pose_graph_optimize_dev", p["trajectory"], ns, None, p["edges"], ns - 1, C.byref(st), p["summary"], host=[(st, pgo_struct(max_iterations=1))])
        off = (np.arange(ns + 1) * N).astype(np.uint64)
        run.raw("cloud_map_add_clouds_dev", cmap._handle(), p["deskewed"], 3, sz(off), ns, p["trajectory"], host=[(off, off // 2)])
        run.raw("cloud_map_emit_dev", cmap._handle(), 1, p["map_xyz"], None, None, self.CAPACITY, p["map_n"])
        off = (np.arange(ns + 1) * N).astype(np.uint64)
        run.raw("occupancy_add_clouds_dev", omap._handle(), p["deskewed"], 3, sz(off), ns, p["trajectory"], host=[(off, off // 2)])
        run.raw("occupancy_query_dev", omap._handle(), p["map_xyz"], 3, self.CAPACITY, p["q_counts"], p["q_state"])
        st = capi.VisibilityParams(min_through=1).struct()
        run.raw("visibility_votes_dev", layout._handle(), p["map_xyz"], 3, self.CAPACITY, p["deskewed"], ns, p["trajectory"], C.byref(st), 0, p["votes"])
        run.raw("visibility_filter_dev", p["votes"], self.CAPACITY, C.byref(st), None, 3, p["dynamic"], None, None, 0, p["n_static"])

    def check(self, got, A):
        assert got["map_n"][0] > 100, got["map_n"]


def test_chain_of_twelve_calls_behind_one_gate():
    SC.gated(Chain())


# ---- switching streams --------------------------------------------------------------------------------------------------------------
def test_set_stream_completes_the_old_stream_and_objects_move_with_the_context():
    """A gated call on s1, then loamx_ctx_set_stream(s2): the header's wording ("the context's stream" is one stream at a time, and
    the call synchronises the one it leaves) means the work on s1 is complete when it returns. A cloud map, an occupancy map, a
    place database, a scan layout and a target index created under s1 give the same bytes under s2 and under the private stream
    (handle 0), which loamx_ctx_synchronize then covers."""
    import torch
    cycles, gate_ms = SC.gate()
    ctx = capi.Context(0)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    objs = []
    try:
        assert s1.cuda_stream != 0 and s2.cuda_stream != 0 and s1.cuda_stream != s2.cuda_stream
        ctx.set_stream(s1.cuda_stream)
        case = Compose(65)
        A, B = case.inputs("A", ctx), case.inputs("B", ctx)
        bufs = SC.Buffers(case, A)
        want_a, want_b = SC.plain(case, ctx, bufs, A), SC.plain(case, ctx, bufs, B)
        assert not SC.same(want_a["trajectory"], want_b["trajectory"])
        # objects made under s1
        layout = ctx.scan_layout(lidar(16, 128))
        cmap, omap, db = ctx.cloud_map(max_voxels=1 << 14), ctx.occupancy_map(max_voxels=1 << 18), place_db_70(ctx)
        objs += [layout, cmap, omap, db]
        clouds = posed_clouds("A", np.float64, 14)
        feats = FeatureBatch().inputs("A", ctx)
        te, tp = feats["tgt_edge"][0, :feats["n_tgt_edge"][0]], feats["tgt_planar"][0, :feats["n_tgt_planar"][0]]
        se, sp = feats["src_edge"][0, :feats["n_src_edge"][0]], feats["src_planar"][0, :feats["n_src_planar"][0]]
        index = ctx.target_index(te, tp, reg_params())
        queries = PLACE.random_descriptors(np.random.default_rng(19), 3, R_, S_)

        def use():
            """one use of each object through the host forms (they run on the context's stream and synchronise it)"""
            cmap.clear(), omap.clear()
            for c in range(2):
                cmap.add_cloud(clouds["points"][3000 * c:3000 * (c + 1)], clouds["poses"][c])
                omap.add_cloud(clouds["points"][3000 * c:3000 * (c + 1)], clouds["poses"][c])
            out = list(cmap.emit()[:3]) + list(omap.query(clouds["points"][:500])) + [db.search(queries, K_)]
            out += list(ctx.organize_cloud(clouds["points"][:3000], layout))
            pose, term, iters = ctx.register_features_indexed(index, se, sp, reg=reg_params())
            return out + [np.asarray(pose), np.array([term, iters])]

        under_s1 = use()
        # the gated call on s1, then the switch
        bufs.load(B)
        bufs.stage(A)
        with torch.cuda.stream(s1):
            torch.cuda._sleep(cycles)
            bufs.dev["results"].copy_(bufs.pin_in["results"], non_blocking=True)
            case.call(SC.Run(ctx, bufs.p), None)
            bufs.pin_out["trajectory"].copy_(bufs.dev["trajectory"], non_blocking=True)
        ctx.set_stream(s2.cuda_stream)
        assert s1.query(), "loamx_ctx_set_stream returned while work was still pending on the stream it left"
        assert SC.same(bufs.read_pinned()["trajectory"], want_a["trajectory"])
        under_s2 = use()
        # a call on s2, then back to the private stream: the switch completes s2 as well, and synchronize covers the private stream
        bufs.load(A)
        case.call(SC.Run(ctx, bufs.p), None)
        ctx.set_stream(0)
        assert s2.query()
        assert SC.same(bufs.read_sync()["trajectory"], want_a["trajectory"])
        bufs.load(B)
        case.call(SC.Run(ctx, bufs.p), None)
        ctx.synchronize()
        out = {k: bufs.dev[k].cpu().numpy()[:want_b[k].nbytes] for k in ("trajectory",)}  # (no torch synchronisation in front of it)
        assert SC.same(out["trajectory"], want_b["trajectory"]), "loamx_ctx_synchronize did not cover the private stream"
        under_own = use()
        for i, (a, b, c) in enumerate(zip(under_s1, under_s2, under_own)):
            assert SC.same(a, b) and SC.same(a, c), f"output {i} of the objects made under the first stream differs under another"
        ctx.target_index_destroy(index)
    finally:
        s1.synchronize(), s2.synchronize()
        for o in objs:
            o.close()
        ctx.close()


# ---- the registration rows without the auxiliary streams -------------------------------------------------------------------------
def test_registration_rows_without_the_auxiliary_streams():
    """LOAMX_NO_AUX_STREAM is read when a context is created: a fresh child process runs the registration rows with it set"""
    env = dict(os.environ, LOAMX_NO_AUX_STREAM="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "registration-rows"], env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert f"{len(REGISTRATION_ROWS)} registration rows ok without the auxiliary streams" in out.stdout, out.stdout[-3000:]


if __name__ == "__main__":
    assert sys.argv[1:] == ["registration-rows"] and os.environ.get("LOAMX_NO_AUX_STREAM") == "1"
    for row in REGISTRATION_ROWS:
        SC.gated(row)
    print(f"{len(REGISTRATION_ROWS)} registration rows ok without the auxiliary streams")
