"""The registration information matrix through the layers above the C ABI: the pybind module `loam` and the C++ header shim
(tests/cpp/test_information_shim.cpp, built with g++ and run as a child process) return the C ABI's record on one 16 x 256
scan pair; covariance() equals the numpy helper's."""
import os
import subprocess
import sys

import numpy as np
import pytest

import info_common as I
from loam_amd import build as B
from loam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 16, 256


def _loam():
    B.build_pybind()
    if B.PY_DIR not in sys.path:
        sys.path.insert(0, B.PY_DIR)
    import loam
    return loam


def build_information_shim_test():
    B.build()
    exe = os.path.join(ROOT, "tests", "cpp", "test_information_shim")
    src = os.path.join(ROOT, "tests", "cpp", "test_information_shim.cpp")
    cmd = ["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", B.LIB_DIR, "-lloamx",
           "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{B.LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def test_information_shim_compiles_without_gpu():
    build_information_shim_test()


def test_python_module_exports_the_information_api_without_gpu():
    loam = _loam()
    assert callable(loam.registrationInformation)
    for name in ("information", "eigenvalues", "eigenvectors", "gradient", "weighted_sq_error", "n_edge", "n_plane", "n_huber",
                 "n_dropped", "covariance", "degenerateDirections"):
        assert hasattr(loam.RegistrationInformation, name), name


@pytest.mark.gpu
def test_information_through_cpp_shim():
    exe = build_information_shim_test()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:]
    assert "0 failures" in out.stdout


@pytest.mark.gpu
def test_information_through_the_python_module():
    from gpu_common import ctx
    loam = _loam()
    A, Bs = capi.synth_scan_host(3, 2, 0, H, W, 0.01), capi.synth_scan_host(3, 2, 1, H, W, 0.01)
    lp = loam.LidarParams(H, W, 1.0, 120.0)
    target, source = loam.extractFeatures(A, lp), loam.extractFeatures(Bs, lp)
    pose = loam.registerFeatures(source, target, loam.Pose3d.Identity())
    got = loam.registrationInformation(source, target, pose)
    se, sp = np.asarray(source.edge_points, dtype=np.float64), np.asarray(source.planar_points, dtype=np.float64)
    te, tp = np.asarray(target.edge_points, dtype=np.float64), np.asarray(target.planar_points, dtype=np.float64)
    q, t = pose.rotation, pose.translation
    pose7 = np.array([q.x(), q.y(), q.z(), q.w(), t[0], t[1], t[2]])
    want = ctx().registration_information(se, sp, te, tp, pose=pose7)
    assert int(want.n_plane) > 500 and int(want.n_edge) > 30

    def same(g):
        return (np.array_equal(g.information, want.information) and np.array_equal(g.eigenvalues, want.eigenvalues)
                and np.array_equal(g.eigenvectors, want.eigenvectors) and np.array_equal(g.gradient, want.gradient)
                and g.weighted_sq_error == want.weighted_sq_error
                and (g.n_edge, g.n_plane, g.n_huber, g.n_dropped) == (want.n_edge, want.n_plane, want.n_huber, want.n_dropped))
    assert same(got)
    assert same(loam.registrationInformation(source, loam.TargetIndex(target), pose))
    ref = I.covariance_numpy(want.information, want.weighted_sq_error, int(want.n_edge) + int(want.n_plane))
    assert np.abs(got.covariance() - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.abs(want.covariance() - ref).max() <= 1e-12 * np.abs(ref).max()
    assert got.degenerateDirections(100.0).shape == (0, 6)
    assert np.array_equal(got.degenerateDirections(got.eigenvalues[1] * 1.0001), want.eigenvectors[:2])
    with pytest.raises(ValueError):
        loam.registrationInformation(loam.LoamFeatures(), target, pose).covariance()
