"""The scan segmentation through the layers above the C ABI: the pybind module `loam` (SegmentationParams, segmentScan) and the
C++ header shim (tests/cpp/test_segment_shim.cpp, built with g++ and run as a child process) return what the C ABI returns on
the same scan, byte for byte, for float and double points; the counts examples/segmented_scans.py prints are reproduced from the
numpy model of tests/segment_common.py."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import segment_common as M
from loam_amd import build as B
from loam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _loam():
    B.build_pybind()
    if B.PY_DIR not in sys.path:
        sys.path.insert(0, B.PY_DIR)
    import loam
    return loam


def build_segment_shim_test():
    B.build()
    exe = os.path.join(ROOT, "tests", "cpp", "test_segment_shim")
    src = os.path.join(ROOT, "tests", "cpp", "test_segment_shim.cpp")
    cmd = ["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", B.LIB_DIR, "-lloamx",
           "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{B.LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def test_segment_shim_compiles_without_gpu():
    build_segment_shim_test()


def test_python_module_exports_the_segmentation_api_without_gpu():
    loam = _loam()
    assert callable(loam.segmentScan)
    p, d = loam.SegmentationParams(), capi.SegmentParams()
    for name in capi.SegmentParams.FIELDS:  # the C ABI's defaults in all three layers
        assert getattr(p, name) == getattr(d, name), name
    assert (d.ground_lines, d.min_cluster_points, d.min_tall_cluster_points, d.min_tall_cluster_lines, d.drop_outliers, d.drop_ground) == (0, 30, 5, 3, 1, 0)
    assert (d.ground_angle, d.segment_angle) == (10.0 * np.pi / 180.0, 60.0 * np.pi / 180.0)
    p.ground_lines, p.segment_angle, p.drop_ground = 7, 0.5, True
    assert (p.ground_lines, p.segment_angle, p.drop_ground) == (7, 0.5, True)
    tg2, c2 = capi.segment_constants()
    assert tg2 == np.tan(d.ground_angle) ** 2 and c2 == np.cos(d.segment_angle) ** 2 and 0.031 < tg2 < 0.0312 and 0.25 < c2 < 0.2500001
    for bad in (dict(ground_angle=np.nan), dict(ground_angle=np.pi / 2), dict(segment_angle=0.0), dict(segment_angle=np.inf)):
        with pytest.raises(capi.LoamxError) as e:
            capi.segment_constants(capi.SegmentParams(**bad))
        assert e.value.status == capi.ERR_BAD_PARAM
    with pytest.raises(TypeError):
        capi.SegmentParams(no_such_field=1)


@pytest.mark.gpu
def test_segment_through_cpp_shim():
    exe = build_segment_shim_test()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:]
    assert "0 failures" in out.stdout


@pytest.mark.gpu
def test_segment_through_the_python_module():
    from gpu_common import ctx
    loam = _loam()
    H, W = 32, 512
    lidar, clidar = loam.LidarParams(H, W, 1.0, 120.0), capi.LidarParams(H, W, 1.0, 120.0)
    settings = (dict(), dict(ground_lines=12, min_cluster_points=10, drop_outliers=False, drop_ground=True, segment_angle=0.6))
    for name in ("canyon", "lot"):
        for scan in (M.real_scan(name), M.real_scan(name, dtype=np.float32)):
            for kw in settings:
                p = loam.SegmentationParams()
                for k, v in kw.items():
                    setattr(p, k, v)
                got = loam.segmentScan(scan, lidar, p)
                want = ctx().segment_scan(scan, clidar, capi.SegmentParams(**kw))
                assert got[3].dtype == scan.dtype and got[3].shape == (H * W, 3) and got[4].shape == (len(want[4]), 4)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
                assert np.array_equal(np.ascontiguousarray(got[3]).view(np.uint8), want[3].view(np.uint8))
                assert np.array_equal(got[4].reshape(-1), want[4].view(np.uint32)) and np.array_equal(got[5], want[5])
                assert len(want[4]) == want[5][4] >= 50
    assert len(loam.segmentScan(M.real_scan("lot"), lidar)) == 6  # (params default)
    with pytest.raises(RuntimeError):
        loam.segmentScan(M.real_scan("lot")[:100], lidar)
    with pytest.raises(RuntimeError):
        bad = loam.SegmentationParams()
        bad.ground_angle = -0.1
        loam.segmentScan(M.real_scan("lot"), lidar, bad)


@pytest.mark.gpu
def test_the_examples_counts_are_the_models():
    from gpu_common import ctx
    spec = importlib.util.spec_from_file_location("segmented_scans_example", os.path.join(ROOT, "examples", "segmented_scans.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    H, W = 32, 512
    for name in ("canyon", "lot"):
        got = example.main(name, H, W, verbose=False, ctx=ctx())
        scan = M.real_scan(name)
        m = M.segment(scan, H, W)
        removed = (m.classes == capi.SEGMENT_OUTLIER)
        lidar = capi.LidarParams(H, W, 1.0, 120.0)
        edge_raw, planar_raw = ctx().extract_features(scan, lidar)
        edge_f, planar_f = ctx().extract_features(m.filtered, lidar)
        want = dict(invalid=m.stats[0], ground=m.stats[1], cluster_cells=m.stats[2], outlier_cells=m.stats[3], accepted=m.stats[4],
                    rejected=m.stats[5], largest=m.stats[6], removed=removed.sum(), edge_raw=len(edge_raw), planar_raw=len(planar_raw),
                    edge_on_removed=removed[edge_raw].sum(), planar_on_removed=removed[planar_raw].sum(), edge_filtered=len(edge_f),
                    planar_filtered=len(planar_f))
        assert got == {k: int(v) for k, v in want.items()}, (name, got, want)
        assert got["removed"] == got["outlier_cells"] > 0 and got["edge_raw"] > 0
