"""The pose-graph optimiser through the layers above the C ABI: the pybind module `loam` (PoseGraphParams, PoseGraphSummary,
PoseGraph) and the C++ header shim (tests/cpp/test_posegraph_shim.cpp, built with g++ and run as a child process) return the C
ABI's bytes on a ring; the defaults are the C ABI's in all three layers; examples/pose_graph.py improves its last pose."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import posegraph_common as G
from loam_amd import build as B
from loam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _loam():
    B.build_pybind()
    if B.PY_DIR not in sys.path:
        sys.path.insert(0, B.PY_DIR)
    import loam
    return loam


def build_posegraph_shim_test():
    B.build()
    exe = os.path.join(ROOT, "tests", "cpp", "test_posegraph_shim")
    src = os.path.join(ROOT, "tests", "cpp", "test_posegraph_shim.cpp")
    cmd = ["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", B.LIB_DIR, "-lloamx",
           "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{B.LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def test_posegraph_shim_compiles_without_gpu():
    build_posegraph_shim_test()


def test_python_module_exports_the_pose_graph_api_with_the_c_abis_defaults_without_gpu():
    loam = _loam()
    for name in ("addPose", "setFixed", "addEdge", "optimize", "pose", "numPoses", "numEdges"):
        assert callable(getattr(loam.PoseGraph, name))
    p, d = loam.PoseGraphParams(), capi.PgoParams()
    st = capi.PgoParamsStruct()
    capi.load().loamx_pgo_default_params(st)
    for name, want in G.DEFAULTS.items():
        assert getattr(p, name) == want == getattr(d, name) == getattr(st, name), name
    p.max_iterations, p.huber_delta = 3, 1.5
    assert (p.max_iterations, p.huber_delta) == (3, 1.5)
    assert [loam.PoseGraphTerminationType(i).name for i in range(6)] == list(capi.PGO_TERMINATIONS)
    for name in ("pose_graph_optimize", "pose_graph_optimize_dev", "pose_graph_linearize", "pose_graph_edges_from_results_dev"):
        assert callable(getattr(capi.Context, name))
    g = loam.PoseGraph()
    assert g.addPose(loam.Pose3d.Identity()) == 0 and g.numPoses() == 1 and g.fixed(0)
    with pytest.raises((RuntimeError, ValueError)):
        g.addEdge(0, 0, loam.Pose3d.Identity(), np.zeros(35))


@pytest.mark.gpu
def test_pose_graph_through_cpp_shim():
    exe = build_posegraph_shim_test()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:]
    assert " 0 failures" in out.stdout


@pytest.mark.gpu
def test_pose_graph_through_the_python_module():
    from gpu_common import ctx
    loam = _loam()
    poses, edges, _ = G.chain_graph(12, 0, 3, closed=True)
    fixed = np.zeros(12, np.uint8)
    fixed[[0, 7]] = 1
    for fx, huber in ((None, 0.0), (fixed, 0.0), (None, 0.5)):
        params = loam.PoseGraphParams()
        params.huber_delta = huber
        g = loam.PoseGraph(params)
        for T in poses:
            g.addPose(loam.Pose3d(loam.Quaterniond(T[3], T[0], T[1], T[2]), T[4:]))
        if fx is not None:
            for i in np.flatnonzero(fx):
                g.setFixed(int(i))
        for e in edges:
            Z = e["a_T_b"]
            g.addEdge(int(e["a"]), int(e["b"]), loam.Pose3d(loam.Quaterniond(Z[3], Z[0], Z[1], Z[2]), Z[4:]), e["information"])
        s = g.optimize()
        want, ws = ctx().pose_graph_optimize(poses, edges, fx, capi.PgoParams(huber_delta=huber))
        got = np.array([[*(getattr(g.pose(i).rotation, c)() for c in "xyzw"), *g.pose(i).translation] for i in range(12)])
        assert got.tobytes() == want.tobytes()
        assert (s.initial_cost, s.final_cost, s.lambda_, s.max_update) == (ws["initial_cost"], ws["final_cost"], ws["lambda"], ws["max_update"])
        assert (s.iterations, s.accepted, s.pcg_iterations, int(s.termination_type), s.n_bad_edges) == \
            (ws["iterations"], ws["accepted"], ws["pcg_iterations"], ws["termination"], 0)
        assert s.termination_type == loam.PoseGraphTerminationType.COST_CONVERGED and s.final_cost < s.initial_cost
    g = loam.PoseGraph()
    g.addPose(loam.Pose3d.Identity())
    g.addPose(loam.Pose3d.Identity())
    g.addEdge(0, 5, loam.Pose3d.Identity(), np.eye(6))
    with pytest.raises(RuntimeError):
        g.optimize()


@pytest.mark.gpu
def test_the_example_improves_its_last_pose():
    _loam()
    spec = importlib.util.spec_from_file_location("pose_graph_example", os.path.join(ROOT, "examples", "pose_graph.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    r = example.main(verbose=False)
    assert r["loop"] == (0, example.N_SCANS - 1)
    assert r["after"] < r["before"], r
    assert r["termination"] in ("COST_CONVERGED", "STEP_CONVERGED")
