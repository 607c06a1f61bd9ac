"""The cloud organiser through the layers above the C ABI: the pybind module `loam` (OrganizeParams, ScanLayout, organizeCloud)
and the C++ header shim (tests/cpp/test_organize_shim.cpp, built with g++ and run as a child process) return what the C ABI
returns on the same cloud, for float and double points, with and without rings; the loop of examples/unordered_cloud.py ends
with the pose the same loop gives on the organised scans, bit for bit."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import organize_common as M
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


def build_organize_shim_test():
    B.build()
    exe = os.path.join(ROOT, "tests", "cpp", "test_organize_shim")
    src = os.path.join(ROOT, "tests", "cpp", "test_organize_shim.cpp")
    cmd = ["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", B.LIB_DIR, "-lloamx",
           "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{B.LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def test_organize_shim_compiles_without_gpu():
    build_organize_shim_test()


def test_python_module_exports_the_organize_api_without_gpu():
    loam = _loam()
    assert callable(loam.organizeCloud) and hasattr(loam, "ScanLayout")
    p = loam.OrganizeParams()
    d = capi.OrganizeParams()
    assert (p.azimuth_zero, p.clockwise, p.keep, p.elevations, p.ring_map) == (0.0, False, loam.OrganizeKeep.First, [], [])
    assert (p.fov_bottom, p.fov_top) == (d.fov_bottom, d.fov_top) == (-np.pi / 12, np.pi / 12)  # the C ABI's defaults in all three layers
    p.keep, p.elevations, p.ring_map = loam.OrganizeKeep.Nearest, [-0.1, 0.1], [1, 0, 0xFFFF]
    assert p.keep == loam.OrganizeKeep.Nearest and p.elevations == [-0.1, 0.1] and p.ring_map == [1, 0, 65535]


@pytest.mark.gpu
def test_organize_through_cpp_shim():
    exe = build_organize_shim_test()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:]
    assert "0 failures" in out.stdout


@pytest.mark.gpu
def test_organize_through_the_python_module():
    from gpu_common import ctx
    loam = _loam()
    H, W = 16, 128
    rng = np.random.default_rng(81)
    pts = M.random_cloud(rng, 4000)
    rings = rng.integers(0, H + 2, len(pts)).astype(np.uint16)
    el = np.sort(rng.uniform(-0.5, 0.3, H))
    for keep, ckeep in ((loam.OrganizeKeep.First, capi.ORGANIZE_KEEP_FIRST), (loam.OrganizeKeep.Nearest, capi.ORGANIZE_KEEP_NEAREST)):
        p = loam.OrganizeParams()
        p.keep, p.elevations, p.clockwise, p.azimuth_zero = keep, list(el), True, 0.3
        layout = loam.ScanLayout(loam.LidarParams(H, W, 1.0, 120.0), p)
        clay = ctx().scan_layout(capi.LidarParams(H, W, 1.0, 120.0), capi.OrganizeParams(0.3, True, ckeep, el))
        try:
            col, tan = clay.tables()
            assert np.array_equal(layout.columnDirections(), col) and np.array_equal(layout.lineTangents(), tan)
            assert (layout.scan_lines, layout.points_per_line) == (H, W)
            for cloud in (pts, pts.astype(np.float32), np.concatenate([pts, np.full((len(pts), 1), np.nan)], axis=1).astype(np.float32)):
                for r in (None, rings):
                    scan, src = loam.organizeCloud(cloud, layout, r)
                    want = ctx().organize_cloud(cloud, clay, r)
                    assert scan.dtype == cloud.dtype and scan.shape == (H * W, 3) and src.dtype == np.uint32
                    assert np.array_equal(M.bits(scan), M.bits(want[0])) and np.array_equal(src, want[1])
                    assert (src != 0xFFFFFFFF).sum() == want[2][0] > 500
            scan, src = loam.organizeCloud(pts, layout, rings=[int(v) for v in rings])  # a list of ints is converted
            assert np.array_equal(src, ctx().organize_cloud(pts, clay, rings)[1])
            with pytest.raises(RuntimeError):
                loam.organizeCloud(pts, layout, rings[:10])
            with pytest.raises((RuntimeError, TypeError)):
                loam.organizeCloud(pts[:, :2], layout)
        finally:
            clay.close()
    with pytest.raises(RuntimeError):
        bad = loam.OrganizeParams()
        bad.elevations = [0.1, 0.0]
        loam.ScanLayout(loam.LidarParams(2, 8, 1.0, 120.0), bad)


@pytest.mark.gpu
def test_the_example_ends_with_the_pose_of_the_loop_on_organised_scans():
    loam = _loam()
    spec = importlib.util.spec_from_file_location("unordered_cloud_example", os.path.join(ROOT, "examples", "unordered_cloud.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    H, W = 32, 512
    got = example.main(H, W, verbose=False)
    lidar_params = loam.LidarParams(H, W, 1.0, 120.0)
    target_scan, source_scan, truth = S.pair("canyon", 0, H, W)
    feats = [loam.extractFeatures(np.ascontiguousarray(s, dtype=np.float32), lidar_params) for s in (target_scan, source_scan)]
    pose = loam.registerFeatures(source=feats[1], target=feats[0], target_T_source_init=loam.Pose3d.Identity())
    q, t = pose.rotation, pose.translation
    want = np.array([q.x(), q.y(), q.z(), q.w(), t[0], t[1], t[2]])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (got, want)
    assert np.linalg.norm(got[4:] - truth[4:]) < 0.05  # (and it is the scene's motion)
