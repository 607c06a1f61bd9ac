"""-m gpu: the pose-graph optimiser on the device against the host build of the same header (tests/hostcheck_posegraph: the whole
solve in the kernels' orders) BY BYTES: linearisation records, final poses and the whole summary, on the smallest graphs at which
each kernel can go wrong; gauge, information and Huber cases; determinism; refusals; the edge kernel; a drive end to end. Then
one LM step of the device against the dense normal equations built from its own linearisation records, every termination code,
a rejected step followed by accepted ones against the model's LM loop, and inner solves capped at odd and even counts."""
import numpy as np
import pytest

import posegraph_common as G
from gpu_common import ctx, option
from loam_amd import capi

pytestmark = pytest.mark.gpu


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def check(poses, edges, fixed=None, **kw):
    """device == host build, by bytes: the linearisation at the start, the final poses, the summary; returns (poses, summary)"""
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
    hd = kw.get("huber_delta", 0.0)
    if len(edges):
        lin = ctx().pose_graph_linearize(poses, edges, hd)
        assert _same(lin, G.host_linearize(poses, edges, hd)), "linearisation records differ"
    got, s = ctx().pose_graph_optimize(poses, edges, fixed, capi.PgoParams(**kw))
    want, ws = G.host_optimize(poses, edges, fixed, **kw)
    assert _same(s, ws), (s, ws)
    assert _same(got, want), "final poses differ"
    assert np.isfinite(got).all()
    return got, s


hub_graph = G.hub_graph


def shaken(graph, seed):
    """an open chain's dead reckoning already has cost ~0: push its free poses off"""
    poses, edges, truth = graph
    rng = np.random.default_rng(seed)
    poses = poses.copy()
    poses[1:] = G.retract(poses[1:], np.concatenate([0.02 * rng.normal(size=(len(poses) - 1, 3)), 0.2 * rng.normal(size=(len(poses) - 1, 3))], axis=1))
    return poses, edges, truth


SHAPES = {
    "two": lambda: shaken(G.chain_graph(2, 0, 1), 101),
    "chain3": lambda: shaken(G.chain_graph(3, 0, 2), 102),
    "ring12": lambda: G.chain_graph(12, 0, 3, closed=True),
    "n257": lambda: G.chain_graph(257, 3, 4),
    "n1025": lambda: G.chain_graph(1025, 10, 5),
    "hub300": lambda: hub_graph(300, 6),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_match_the_host_build_by_bytes(name):
    poses, edges, _ = SHAPES[name]()
    if name == "n257":
        assert len(edges) > 256 and len(poses) > 256
    if name == "n1025":
        assert len(edges) > 1024
    if name == "hub300":
        assert np.bincount(np.concatenate([edges["a"], edges["b"]]))[0] == 300
    kw = dict(max_iterations=4, max_pcg_iterations=150) if name in ("n1025", "hub300") else {}
    got, s = check(poses, edges, **kw)
    assert s["iterations"] >= 1 and s["accepted"] >= 1 and s["final_cost"] < s["initial_cost"] and s["pcg_iterations"] >= 1
    assert _same(got[0], poses[0])


def test_one_pose_and_no_edge():
    poses, edges, _ = G.chain_graph(1, 0, 7)
    got, s = check(poses, edges)
    assert s["termination"] == G.NOTHING_TO_DO and _same(got, poses)
    got, s = check(np.zeros((0, 7)), edges)
    assert s["termination"] == G.NOTHING_TO_DO


def test_duplicate_edges_and_edges_listed_backwards():
    poses, edges, truth = G.chain_graph(20, 4, 8, closed=True)
    assert (edges["b"] < edges["a"]).sum() >= 2
    dup = np.concatenate([edges, edges[[3, 3, 21]]])
    rng = np.random.default_rng(9)
    back = G.make_edges([(8, 7)], G.measured(truth, [(8, 7)], rng), np.diag([100.0] * 6))  # the reverse of edge 7
    got, s = check(poses, np.concatenate([dup, back]))
    assert s["final_cost"] < s["initial_cost"]


def test_gauge():
    poses, edges, _ = G.chain_graph(30, 3, 10, closed=True)
    for fixed_ids in ([14], [29], [0, 14, 29]):
        fx = np.zeros(30, np.uint8)
        fx[fixed_ids] = 1
        got, s = check(poses, edges, fx)
        assert _same(got[fixed_ids], poses[fixed_ids]) and not _same(got, poses)
    fx = np.ones(30, np.uint8)
    fx[11] = 0
    got, s = check(poses, edges, fx)
    moved = np.flatnonzero((got != poses).any(axis=1))
    assert moved.tolist() == [11] and s["accepted"] >= 1
    got, s = check(poses, edges, np.ones(30, np.uint8))
    assert s["termination"] == G.NOTHING_TO_DO and _same(got, poses)


def test_component_without_a_fixed_pose_stays_finite():
    pa, ea, _ = G.chain_graph(9, 1, 11, closed=True)
    pb, eb, _ = G.chain_graph(7, 1, 12, closed=True)
    eb = eb.copy()
    eb["a"] += 9
    eb["b"] += 9
    got, s = check(np.concatenate([pa, pb]), np.concatenate([ea, eb]))  # pose 0 alone is fixed: the second ring floats
    assert s["final_cost"] < s["initial_cost"]


def test_information_cases():
    poses, edges, _ = G.chain_graph(16, 2, 13, closed=True)
    zero = edges.copy()
    zero["information"][5] = 0.0
    check(poses, zero)
    tail = edges[:15].copy()  # an open chain whose last edge carries nothing: the damping floor solves the last pose
    tail["information"][14] = 0.0
    got, s = check(poses, tail)
    rng = np.random.default_rng(14)
    rank3 = edges.copy()
    rank3["information"][:] = np.stack([G.rand_information(rng, rank=3) for _ in edges])
    assert np.linalg.matrix_rank(rank3["information"][0]) == 3
    check(poses, rank3)
    bad = edges.copy()
    bad["a_T_b"][-1, 4] += 5.0
    clean, _ = check(poses, edges)
    plain, _ = check(poses, bad)
    robust, s = check(poses, bad, huber_delta=1.0)
    assert G.pose_distance(robust, clean)[1].max() < G.pose_distance(plain, clean)[1].max()


def test_same_bytes_on_poisoned_workspaces_and_in_any_edge_order():
    poses, edges, _ = G.chain_graph(300, 6, 15)
    kw = dict(max_iterations=3, max_pcg_iterations=60)
    with option("DEBUG_POISON"):
        a = check(poses, edges, **kw)
        b = check(poses, edges, **kw)
    assert _same(a[0], b[0]) and _same(a[1], b[1])
    perm = np.random.default_rng(16).permutation(len(edges))
    c = check(poses, edges[perm], **kw)  # (against the host build run on the same permuted order)
    assert np.abs(c[0] - a[0]).max() < 1e-6


def _dev_call(poses, edges, fixed=None, **kw):
    c = ctx()
    bufs = [c.alloc(max(poses.nbytes, 8)).upload(poses), c.alloc(max(edges.nbytes, 8)).upload(edges), c.alloc(capi.PGO_SUMMARY_DTYPE.itemsize)]
    bufs[2].upload(np.full(capi.PGO_SUMMARY_DTYPE.itemsize, 0xEE, np.uint8))
    fb = c.alloc(len(poses)).upload(np.ascontiguousarray(fixed, np.uint8)) if fixed is not None else None
    try:
        c.pose_graph_optimize_dev(bufs[0], len(poses), bufs[1], len(edges), fb or 0, capi.PgoParams(**kw), bufs[2])
        c.synchronize()
        return bufs[0].download(np.float64, poses.size).reshape(-1, 7), bufs[2].download(capi.PGO_SUMMARY_DTYPE, 1)[0]
    finally:
        for b in bufs + ([fb] if fb else []):
            b.free()


def test_dev_form_refuses_bad_edges_and_goes_on():
    poses, edges, _ = G.chain_graph(40, 3, 17, closed=True)
    for mutate, count in ((lambda e: e["a"].__setitem__(5, 40), 1), (lambda e: e["b"].__setitem__(7, 0xFFFFFFFF), 1),
                          (lambda e: (e["a"].__setitem__(9, e["b"][9]), e["b"].__setitem__(20, 1000)), 2)):
        bad = edges.copy()
        mutate(bad)
        got, s = _dev_call(poses, bad)
        want, ws = G.host_optimize(poses, bad)
        assert s["termination"] == G.BAD_INPUT and s["n_bad_edges"] == count and _same(got, poses) and _same(s, ws)
    got, s = _dev_call(poses, edges)  # the process and the context are healthy afterwards
    want, ws = G.host_optimize(poses, edges)
    assert _same(got, want) and _same(s, ws) and s["termination"] == G.COST_CONVERGED
    fx = np.zeros(40, np.uint8)
    fx[[3, 39]] = 1
    got, s = _dev_call(poses, edges, fx)
    want, ws = G.host_optimize(poses, edges, fx)
    assert _same(got, want) and _same(s, ws)


def test_host_form_refusals():
    poses, edges, _ = G.chain_graph(10, 1, 18, closed=True)
    c = ctx()

    def refused(p=poses, e=edges, f=None, **kw):
        before = np.array(p, copy=True)
        with pytest.raises(capi.LoamxError) as err:
            c.pose_graph_optimize(p, e, f, capi.PgoParams(**kw))
        assert err.value.status == capi.ERR_BAD_PARAM
        assert _same(before, p)

    for field in ("pcg_tolerance", "cost_tolerance", "step_tolerance", "huber_delta"):
        refused(**{field: -1e-3})
        refused(**{field: float("nan")})
    refused(initial_lambda=float("inf"))
    refused(initial_lambda=0.0)
    refused(max_iterations=0)
    refused(f=np.zeros(10, np.uint8))
    for where in ("pose", "measurement", "information"):
        p, e = poses.copy(), edges.copy()
        if where == "pose":
            p[4, 2] = np.nan
        elif where == "measurement":
            e["a_T_b"][2, 6] = np.inf
        else:
            e["information"][1, 0, 5] = np.nan
        refused(p, e)
    for a, b in ((3, 3), (10, 2), (2, 0xFFFFFFFF)):
        e = edges.copy()
        e["a"][4], e["b"][4] = a, b
        refused(e=e)
        with pytest.raises(capi.LoamxError):
            c.pose_graph_linearize(poses, e)
    lib, h = capi.load(), c.h
    st = capi.PgoParams().struct()
    import ctypes as C
    s = np.zeros(1, capi.PGO_SUMMARY_DTYPE)
    assert lib.loamx_pose_graph_optimize(h, None, 10, None, edges.ctypes.data, len(edges), C.byref(st), s.ctypes.data) == capi.ERR_BAD_PARAM
    assert lib.loamx_pose_graph_optimize(h, poses.ctypes.data, 10, None, None, len(edges), C.byref(st), s.ctypes.data) == capi.ERR_BAD_PARAM
    assert lib.loamx_pose_graph_optimize(h, poses.ctypes.data, 10, None, edges.ctypes.data, len(edges), None, s.ctypes.data) == capi.ERR_BAD_PARAM
    assert lib.loamx_pose_graph_optimize(h, poses.ctypes.data, 10, None, edges.ctypes.data, len(edges), C.byref(st), None) == capi.ERR_BAD_PARAM
    e = edges.copy()
    e["information"][:, 3, 1] = np.nan  # (below the diagonal: never read)
    got, s = check(poses, e)
    assert s["termination"] == G.COST_CONVERGED


def test_edges_from_results_against_a_numpy_repack():
    rng = np.random.default_rng(19)
    n = 300
    res = np.zeros(n, capi.RESULT_DTYPE)
    res["pose"] = np.stack([G.rand_pose(rng) for _ in range(n)])
    info = np.zeros(n, capi.INFORMATION_DTYPE)
    info["information"] = np.stack([G.rand_information(rng) for _ in range(n)])
    info["eigenvalues"] = 7.0
    c = ctx()
    bufs = [c.alloc(res.nbytes).upload(res), c.alloc(info.nbytes).upload(info), c.alloc(n * capi.PGO_EDGE_DTYPE.itemsize)]
    try:
        for first in (0, 41):
            bufs[2].upload(np.full(n * capi.PGO_EDGE_DTYPE.itemsize, 0xEE, np.uint8))
            c.pose_graph_edges_from_results_dev(bufs[0], bufs[1], n, bufs[2], first)
            c.synchronize()
            got = bufs[2].download(capi.PGO_EDGE_DTYPE, n)
            want = np.zeros(n, capi.PGO_EDGE_DTYPE)
            want["a"], want["b"] = first + np.arange(n), first + np.arange(n) + 1
            want["a_T_b"], want["information"] = res["pose"], info["information"]
            assert _same(got, want)
    finally:
        for b in bufs:
            b.free()


def test_a_drive_end_to_end():
    """sequence with information -> edges -> one loop edge -> optimise, on the 12-scan lot drive at 32 x 512 (examples/pose_graph.py
    run on the shared context): the last pose ends nearer the truth than the composed odometry, and the solve on the device is the
    host build's on the same edges"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "pose_graph.py")
    spec = importlib.util.spec_from_file_location("pose_graph_drive", path)
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    r = example.main(scan_lines=32, points_per_line=512, verbose=False, ctx=ctx())
    assert r["loop"] == (0, 11) and r["odometry"].shape == (12, 7)
    print(f"last pose: {r['before']:.4f} m from the truth before, {r['after']:.4f} m after; {r['summary']}")
    assert r["after"] < r["before"]
    assert r["summary"]["accepted"] >= 1 and r["summary"]["final_cost"] < r["summary"]["initial_cost"]
    assert _same(r["corrected"][0], r["odometry"][0]) and _same(r["odometry"][0], r["truth"][0])
    want, ws = G.host_optimize(r["odometry"], r["edges"])
    assert _same(r["corrected"], want) and _same(r["summary"], ws)
    assert np.array_equal(r["edges"]["a"], np.r_[np.arange(11), 0]) and np.array_equal(r["edges"]["b"], np.r_[np.arange(1, 12), 11])


# ---- one LM step, the terminations and the trace on the device (the models and figures: tests/posegraph_common.py) ---------------
ONE_STEP = dict(max_iterations=1, cost_tolerance=0.0, step_tolerance=0.0)


def _linearize(poses, edges, huber_delta=0.0):
    return ctx().pose_graph_linearize(poses, edges, huber_delta)


@pytest.mark.parametrize("name", ["ring12", "ring40_fixed_7_22", "ring40_outlier_huber", "hub300"])
def test_the_device_step_satisfies_the_stopping_rule_and_is_the_dense_step(name):
    """G.check_step on the device's own poses and its own linearisation records. hub300 (301 poses, 599 edges: two workgroups,
    chunked sums) ends by tolerance after 47 and 72 of at most 500 PCG iterations."""
    poses, edges, fixed, hd = G.STEP_GRAPHS[name]()
    if name == "hub300":
        assert len(poses) > 256 and len(edges) > 256
    for tol in (1e-8, 1e-12):
        out, s = check(poses, edges, fixed, pcg_tolerance=tol, huber_delta=hd, **ONE_STEP)
        fig = G.check_step(name, poses, edges, fixed, hd, _linearize(poses, edges, hd), out, s, tol, min(500, 6 * len(poses)))
        assert fig["by_tolerance"]


def test_every_termination_code_on_the_device():
    poses, edges, _ = G.chain_graph(12, 1, seed=30, closed=True)
    out, s = check(poses, edges)
    assert s["termination"] == G.COST_CONVERGED and s["accepted"] >= 1 and s["final_cost"] < s["initial_cost"]
    _, s1 = check(poses, edges, max_iterations=1, cost_tolerance=0.0)
    assert s1["termination"] == G.MAX_ITERATIONS and s1["iterations"] == 1 and s1["accepted"] == 1
    # a rejected step leaves the poses as they were
    far, far_edges = G.shaken_ring12()
    out0, s0 = check(far, far_edges, **ONE_STEP)
    assert s0["termination"] == G.MAX_ITERATIONS and s0["accepted"] == 0 and s0["lambda"] == 10.0 * G.DEFAULTS["initial_lambda"] and _same(out0, far)
    assert s0["final_cost"] == s0["initial_cost"] and s0["pcg_iterations"] >= 1 and s0["max_update"] > 0.0
    # at the minimum every step is rejected until lambda passes 1e12 ...
    best, _ = check(poses, edges, max_iterations=100, cost_tolerance=0.0, step_tolerance=0.0, pcg_tolerance=1e-12)
    out2, s2 = check(best, edges, max_iterations=100, cost_tolerance=0.0, step_tolerance=0.0, initial_lambda=1e9)
    assert s2["termination"] == G.LAMBDA_OVERFLOW and s2["lambda"] > 1e12 and s2["iterations"] < 100
    assert s2["accepted"] == 0 and _same(out2, best)
    # ... unless the step is already below the step tolerance
    out3, s3 = check(best, edges, step_tolerance=1e-3)
    assert s3["termination"] == G.STEP_CONVERGED and s3["iterations"] == 1 and s3["accepted"] == 0 and _same(out3, best)
    assert 0.0 < s3["max_update"] <= 1e-3 and s3["pcg_iterations"] >= 1


def test_a_rejected_step_followed_by_an_accepted_one():
    """the shaken ring12 iteration by iteration (solves of 1 .. 8 iterations, the prefix property between device runs by bytes)
    against G.lm_model on the device's linearisation records: two rejections, then acceptances"""
    accepted = G.check_trace("ring12_shaken", check, _linearize)
    assert accepted[:3] == [0, 0, 1]


@pytest.mark.parametrize("name", ["ring12", "hub300"])
def test_capped_inner_solves_of_both_parities_then_further_iterations(name):
    """max_pcg_iterations 1, 2, 3, 7: the inner solve stops at its cap with the direction in either of the launcher's two arrays
    and the state in either copy, and three more LM iterations follow. By bytes against the host build; the first step also
    against G.pcg_model."""
    poses, edges, fixed, hd = G.STEP_GRAPHS[name]()
    H, g, free = G.dense_system(poses, edges, fixed, G.DEFAULTS["initial_lambda"], hd, _linearize(poses, edges, hd))
    for k in (1, 2, 3, 7):
        out, s = check(poses, edges, fixed, max_iterations=4, max_pcg_iterations=k)
        assert s["iterations"] == 4 and s["pcg_iterations"] == 4 * k and s["accepted"] >= 2 and s["final_cost"] < s["initial_cost"]
        first, s1 = check(poses, edges, fixed, max_pcg_iterations=k, **ONE_STEP)
        ref, it, why = G.pcg_model(H, g, k, G.DEFAULTS["pcg_tolerance"])
        d = G.relative(G.step_of(poses, first)[free].ravel(), ref)
        print(f"{name} k {k}: first step against the model {d:.3g}; {s}")
        assert (it, why) == (k, "cap") and s1["pcg_iterations"] == k and s1["accepted"] == 1
        assert d <= G.TRUNCATED_REL_BOUND
