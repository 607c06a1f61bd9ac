"""The surfel map through the layers above the C ABI: the ctypes layer (capi.SurfelMap), the pybind module `loam`
(SurfelMapParams, SurfelMap) and the C++ header shim (tests/cpp/test_surfel_shim.cpp, built with g++ and run as a child process)
against the Python model of tests/surfel_common.py on the same small input; the defaults are the C ABI's in every layer."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import outdoor_scenes as S
import surfel_common as M
from loam_amd import build as B
from loam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _loam():
    B.build_pybind()
    if B.PY_DIR not in sys.path:
        sys.path.insert(0, B.PY_DIR)
    import loam
    return loam


def build_surfel_shim_test():
    B.build()
    exe = os.path.join(ROOT, "tests", "cpp", "test_surfel_shim")
    src = os.path.join(ROOT, "tests", "cpp", "test_surfel_shim.cpp")
    cmd = ["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", B.LIB_DIR, "-lloamx",
           "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{B.LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def test_surfel_shim_compiles_without_gpu():
    build_surfel_shim_test()


def test_every_layer_exports_the_surfel_map_with_the_c_abis_defaults_without_gpu():
    loam = _loam()
    assert hasattr(loam, "SurfelMap") and hasattr(loam, "SurfelMapParams")
    for name in ("add", "clear", "surfels", "query", "stats"):
        assert callable(getattr(loam.SurfelMap, name))
    p, d = loam.SurfelMapParams(), capi.SurfelMapParams()
    st = capi.SurfelMapParamsStruct()
    capi.load().loamx_default_surfel_map_params(st)
    assert (p.leaf, p.min_range, p.max_range) == M.DEFAULTS == (d.leaf, d.min_range, d.max_range) == (st.leaf, st.min_range, st.max_range)
    p.leaf = 0.4
    assert p.leaf == 0.4
    assert capi.SURFEL_DTYPE.itemsize == 128 and capi.SURFEL_DTYPE == M.SURFEL_DTYPE
    assert capi.SURFEL_MAP_STATS_DTYPE.itemsize == 56 and capi.SURFEL_MAP_STATS_DTYPE.names == M.STAT_NAMES
    for name in ("add_clouds_dev", "add_cloud", "emit_dev", "emit", "query_dev", "query", "clear", "stats", "claims", "close"):
        assert callable(getattr(capi.SurfelMap, name))
    assert callable(capi.Context.surfel_map)
    # size checks raise ValueError before the handle or the library is looked at
    closed = type("NoMap", (), {"max_voxels": 4})()
    for bad in (dict(capacity=-1), dict(capacity=1, min_points=-1), dict(capacity=1, min_points=1 << 32)):
        with pytest.raises(ValueError):
            capi.SurfelMap.emit_dev(closed, d_n_out=0, **bad)
        with pytest.raises(ValueError):
            capi.SurfelMap.emit(closed, **bad)
    with pytest.raises(ValueError):
        capi.SurfelMap.query_dev(None, 0, -3, 1)
    with pytest.raises(ValueError):
        capi.SurfelMap.query(None, np.zeros((3, 2)))


@pytest.mark.gpu
def test_surfel_map_through_cpp_shim():
    exe = build_surfel_shim_test()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:]
    assert " 0 failures" in out.stdout


@pytest.mark.gpu
def test_surfel_map_through_the_python_module_and_the_ctypes_layer():
    from gpu_common import ctx
    loam = _loam()
    H, W = 16, 256
    p = loam.SurfelMapParams()
    p.leaf, p.max_range = 0.8, 60.0
    m = loam.SurfelMap(p, 1 << 14)
    cm = ctx().surfel_map(capi.SurfelMapParams(0.8, None, 60.0), 1 << 14)
    model = M.SurfelMapModel(0.8, 0.5, 60.0)
    try:
        assert (m.params.leaf, m.params.min_range, m.params.max_range, m.max_voxels) == (0.8, 0.5, 60.0, 1 << 14)
        for rounds in range(2):
            for i, name in enumerate(S.SCENES):
                o, yaw = S.sensor_origin(name, 0)
                scan = S.scan_at(name, 0, o, yaw, H, W, noise_seed=1)
                pose7 = S.yaw_pose(yaw, o)
                pose = loam.Pose3d(loam.Quaterniond(pose7[3], pose7[0], pose7[1], pose7[2]), pose7[4:])
                back = np.array([pose.rotation.x(), pose.rotation.y(), pose.rotation.z(), pose.rotation.w(), *pose.translation])
                for cloud in (scan, scan.astype(np.float32), np.concatenate([scan, np.ones((len(scan), 1))], axis=1)):
                    m.add(cloud, pose)
                    cm.add_cloud(cloud, back)
                    model.add(cloud, poses=back[None])
                m.add(scan[:100])
                cm.add_cloud(scan[:100])
                model.add(scan[:100])
            for min_points in (1, 4):
                want, n = model.emit(min_points)
                rec, n_c = cm.emit(min_points)
                M.assert_emit_equal((rec, n_c), (want, n), ("ctypes", rounds, min_points))
                got = m.surfels(min_points)
                assert got["mean"].dtype == np.float64 and got["count"].dtype == np.uint32 and got["first"].dtype == np.uint32
                for field in M.SURFEL_DTYPE.names:
                    assert M.same_bytes(got[field], np.ascontiguousarray(want[field])), ("pybind", field, rounds, min_points)
                assert n > 100 and (got["count"] >= min_points).all()
                q = np.concatenate([want["mean"][:200] + 0.01, [[500.0, 0.0, 0.0]]])
                w_rec, w_dist, w_cnt = model.query(q, min_points)
                c_rec, c_dist, c_cnt = cm.query(q, min_points)
                M.assert_records_equal(c_rec, w_rec, "ctypes query")
                assert M.same_bytes(c_dist, w_dist) and M.same_bytes(c_cnt, w_cnt) and (w_cnt[:-1] > 0).any() and w_cnt[-1] == 0
                pq = m.query(q, min_points)
                for field in M.SURFEL_DTYPE.names:
                    assert M.same_bytes(pq[field], np.ascontiguousarray(w_rec[field])), ("pybind query", field)
                assert M.same_bytes(pq["distance"], w_dist)
            st = m.stats()
            M.assert_stats_equal(st, model.stats())
            M.assert_stats_equal(cm.stats(), model.stats())
            assert st["points_offered"] == 3 * (3 * H * W + 100) and st["overflow"] == 0
            m.clear(), cm.clear(), model.clear()
            assert m.stats()["voxels"] == 0 and len(m.surfels()["count"]) == 0
        with pytest.raises((RuntimeError, TypeError)):
            m.add(np.zeros((5, 2)))
        with pytest.raises(RuntimeError):
            bad = loam.SurfelMapParams()
            bad.leaf = -1.0
            loam.SurfelMap(bad)
    finally:
        cm.close()


@pytest.mark.gpu
def test_the_example_fills_its_map_at_the_corrected_poses_and_its_figures_are_the_models():
    _loam()
    spec = importlib.util.spec_from_file_location("surface_normals_example", os.path.join(ROOT, "examples", "surface_normals.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    out = example.main(scan_lines=16, points_per_line=256, verbose=False)
    n = example.N_SCANS
    assert out["scans"].shape == (n, 16 * 256, 3) and out["scans"].dtype == np.float32
    assert M.same_bytes(out["poses"], out["drive"]["corrected"])
    model = M.SurfelMapModel(out["leaf"])
    model.add(out["scans"].reshape(-1, 3), np.arange(n + 1) * (16 * 256), out["poses"])
    want, n_vox = model.emit(example.MIN_POINTS)
    assert out["voxels"] == n_vox > 300
    M.assert_records_equal(out["surfels"], want, "the example's map")
    M.assert_stats_equal(out["stats"], model.stats())
    w_rec, w_dist, w_cnt = model.query(out["query_points"], example.MIN_POINTS)
    M.assert_records_equal(out["query_records"], w_rec, "the example's query")
    assert M.same_bytes(out["query_distance"], w_dist) and M.same_bytes(out["query_count"], w_cnt)
    # the figures it prints: the lot is mostly ground, its normals point up, and the last scan lies on the map it is part of
    assert out["flat_share"] > 0.5 and out["ground_voxels"] > 100 and out["ground_angle_deg"] < 1.0
    assert out["found"] > 0.5 * out["queried"] and out["mean_abs_distance"] < 0.1
