"""The cloud map through the layers above the C ABI: the pybind module `loam` (CloudMapParams, CloudMap) and the C++ header shim
(tests/cpp/test_cloudmap_shim.cpp, built with g++ and run as a child process) return the C ABI's bytes on the same small input;
the defaults are the C ABI's in all three layers; examples/global_map.py assembles its two maps, and the one at the corrected
poses is the numpy model's on the poses and scans the example downloaded."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import cloudmap_common as M
import outdoor_scenes as S
from loam_amd import build as B
from loam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _loam():
    B.build_pybind()
    if B.PY_DIR not in sys.path:
        sys.path.insert(0, B.PY_DIR)
    import loam
    return loam


def build_cloudmap_shim_test():
    B.build()
    exe = os.path.join(ROOT, "tests", "cpp", "test_cloudmap_shim")
    src = os.path.join(ROOT, "tests", "cpp", "test_cloudmap_shim.cpp")
    cmd = ["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", B.LIB_DIR, "-lloamx",
           "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{B.LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def test_cloudmap_shim_compiles_without_gpu():
    build_cloudmap_shim_test()


def test_python_module_exports_the_cloud_map_api_with_the_c_abis_defaults_without_gpu():
    loam = _loam()
    assert hasattr(loam, "CloudMap") and hasattr(loam, "CloudMapParams")
    for name in ("add", "clear", "points", "stats"):
        assert callable(getattr(loam.CloudMap, name))
    p, d = loam.CloudMapParams(), capi.CloudMapParams()
    st = capi.CloudMapParamsStruct()
    capi.load().loamx_default_cloud_map_params(st)
    assert (p.leaf, p.min_range, p.max_range) == M.DEFAULTS == (d.leaf, d.min_range, d.max_range) == (st.leaf, st.min_range, st.max_range)
    p.leaf = 0.4
    assert p.leaf == 0.4
    assert capi.CLOUD_MAP_STATS_DTYPE.itemsize == 56 and capi.CLOUD_MAP_STATS_DTYPE.names == M.STAT_NAMES
    for name in ("add_clouds_dev", "add_cloud", "emit_dev", "emit", "clear", "stats", "claims", "close"):
        assert callable(getattr(capi.CloudMap, name))
    assert callable(capi.Context.cloud_map)
    names = [capi.load().loamx_kernel_name(i).decode() for i in range(capi.K_COUNT)]
    assert names[capi.K_CLOUD_ACCUMULATE:] == ["cloud_accumulate_kernel", "cloud_accumulate_plain_kernel", "cloud_list_kernels", "cloud_emit_kernels"]


@pytest.mark.gpu
def test_cloud_map_through_cpp_shim():
    exe = build_cloudmap_shim_test()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:]
    assert " 0 failures" in out.stdout


@pytest.mark.gpu
def test_cloud_map_through_the_python_module():
    from gpu_common import ctx
    loam = _loam()
    H, W = 16, 256
    p = loam.CloudMapParams()
    p.leaf, p.max_range = 0.4, 60.0
    m = loam.CloudMap(p, 1 << 14)
    cm = ctx().cloud_map(capi.CloudMapParams(0.4, None, 60.0), 1 << 14)
    try:
        assert (m.params.leaf, m.params.min_range, m.params.max_range, m.max_voxels) == (0.4, 0.5, 60.0, 1 << 14)
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
                m.add(scan[:100])
                cm.add_cloud(scan[:100])
            for min_points in (1, 4):
                xyz, counts, first = m.points(min_points)
                assert xyz.dtype == np.float64 and counts.dtype == np.uint32 and first.dtype == np.uint32
                want = cm.emit(min_points)
                M.assert_emit_equal((xyz, counts, first, len(counts)), want, (rounds, min_points))
                assert len(counts) > 100 and (counts >= min_points).all()
            st = m.stats()
            M.assert_stats_equal(st, cm.stats())
            assert st["points_offered"] == 3 * (3 * H * W + 100) and st["overflow"] == 0
            m.clear(), cm.clear()
            assert m.stats()["voxels"] == 0 and len(m.points()[1]) == 0
        with pytest.raises((RuntimeError, TypeError)):
            m.add(np.zeros((5, 2)))
        with pytest.raises(RuntimeError):
            bad = loam.CloudMapParams()
            bad.leaf = -1.0
            loam.CloudMap(bad)
    finally:
        cm.close()


@pytest.mark.gpu
def test_the_example_assembles_its_maps_and_the_corrected_one_is_the_models():
    _loam()
    spec = importlib.util.spec_from_file_location("global_map_example", os.path.join(ROOT, "examples", "global_map.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    out = example.main(scan_lines=16, points_per_line=256, verbose=False)
    n = example.N_SCANS
    assert out["deskewed"].shape == (n, 16 * 256, 3) and out["deskewed"].dtype == np.float32
    for stage in ("odometry", "corrected"):
        model = M.CloudMapModel(out["leaf"])
        model.add(out["deskewed"].reshape(-1, 3), np.arange(n + 1) * (16 * 256), out[stage + "_poses"])
        xyz, count, first, n_vox = model.emit()
        assert out[stage + "_voxels"] == n_vox > 1000
        assert M.same_bytes(out[stage + "_cloud"], xyz), stage
        M.assert_stats_equal(out[stage + "_stats"], model.stats(), stage)
    assert M.same_bytes(out["corrected_poses"], out["drive"]["corrected"]) and M.same_bytes(out["odometry_poses"], out["drive"]["odometry"])
    assert not M.same_bytes(out["corrected_poses"], out["odometry_poses"])
