"""Surfel localisation through the layers above the C ABI: the ctypes layer (capi.SurfelLocalizer), the pybind module `loam`
(LocalizeParams, LocalizeResult, SurfelMap.localize) and the C++ header shim (tests/cpp/test_localize_shim.cpp, built with g++ and
run as a child process), checked against the ctypes layer by bytes; the defaults are the C ABI's in every layer."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import localize_common as L
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


def build_localize_shim_test():
    B.build()
    exe = os.path.join(ROOT, "tests", "cpp", "test_localize_shim")
    src = os.path.join(ROOT, "tests", "cpp", "test_localize_shim.cpp")
    cmd = ["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", B.LIB_DIR, "-lloamx",
           "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{B.LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def test_localize_shim_compiles_without_gpu():
    build_localize_shim_test()


def test_every_layer_exports_the_localiser_with_the_c_abis_defaults_without_gpu():
    loam = _loam()
    assert hasattr(loam, "LocalizeParams") and hasattr(loam, "LocalizeResult") and callable(loam.SurfelMap.localize)
    p, d = loam.LocalizeParams(), capi.LocalizeParams()
    st = capi.LocalizeParamsStruct()
    capi.load().loamx_default_localize_params(st)
    for name in L.PARAM_NAMES:
        assert getattr(p, name) == getattr(d, name) == getattr(st, name) == L.DEFAULTS[name], name
    p.neighborhood = 1
    assert p.neighborhood == 1
    assert capi.LOCALIZE_RESULT_DTYPE.itemsize == 128 and capi.LOCALIZE_RESULT_DTYPE == L.RESULT_DTYPE
    for name in ("run_dev", "run", "close"):
        assert callable(getattr(capi.SurfelLocalizer, name))
    assert callable(capi.SurfelMap.localizer)
    # size and dtype checks raise ValueError before the handle or the library is looked at
    with pytest.raises(ValueError):
        capi.SurfelLocalizer.run(None, np.zeros((3, 2)), np.zeros(7))
    with pytest.raises(ValueError):
        capi.SurfelLocalizer.run(None, np.zeros((3, 3)), np.zeros(6))
    with pytest.raises(ValueError):
        capi.SurfelLocalizer.run_dev(None, 0, -3, [0, 1], 0, 0, 0)
    with pytest.raises(ValueError):
        capi.SurfelLocalizer.run_dev(None, 0, 3, [[0, 1]], 0, 0, 0)
    with pytest.raises(ValueError):
        capi.LocalizeParams(max_iterations=-1).struct()
    with pytest.raises(ValueError):
        capi.LocalizeParams(no_such_parameter=1)


@pytest.mark.gpu
def test_localize_through_cpp_shim():
    exe = build_localize_shim_test()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:]
    assert " 0 failures" in out.stdout


@pytest.mark.gpu
def test_localize_through_the_python_module_and_the_ctypes_layer():
    from gpu_common import ctx
    loam = _loam()
    scans, poses = L.drive("lot")
    mp = loam.SurfelMapParams()
    m = loam.SurfelMap(mp, 1 << 15)
    cm = ctx().surfel_map(capi.SurfelMapParams(), 1 << 15)
    loc = cm.localizer(1, 4096)

    def pose3d(p7):
        return loam.Pose3d(loam.Quaterniond(p7[3], p7[0], p7[1], p7[2]), p7[4:])

    def back(pose):
        return np.array([pose.rotation.x(), pose.rotation.y(), pose.rotation.z(), pose.rotation.w(), *pose.translation])

    try:
        for i in range(6):
            pose = pose3d(poses[i])
            m.add(scans[i], pose)
            cm.add_cloud(scans[i], back(pose))
        for kw in (dict(), dict(neighborhood=1, max_iterations=2, huber_delta=0.0, min_eigenvalue_per_row=0.01), dict(max_iterations=0)):
            p = loam.LocalizeParams()
            for k, v in kw.items():
                setattr(p, k, v)
            init = pose3d(L.displaced(poses[6]))
            for cloud in (scans[6], scans[6].astype(np.float32), np.concatenate([scans[6], np.ones((4096, 1))], axis=1)):
                got_pose, got, info = m.localize(cloud, init, p)
                want_pose, want, want_info = loc.run(cloud, back(init), capi.LocalizeParams(**kw))
                assert got.tobytes() == want.tobytes(), kw
                assert M.same_bytes(got.pose.reshape(7), want_pose)
                assert M.same_bytes(np.ascontiguousarray(info.information), np.ascontiguousarray(want_info["information"]))
                assert M.same_bytes(np.ascontiguousarray(info.eigenvalues).reshape(6), np.ascontiguousarray(want_info["eigenvalues"]))
                assert M.same_bytes(np.ascontiguousarray(info.gradient).reshape(6), np.ascontiguousarray(want_info["gradient"]))
                assert (info.n_edge, info.n_plane, info.n_huber, info.n_dropped) == (0, want["n_rows"], want["n_huber"], 0)
                assert M.same_bytes(back(got_pose), back(pose3d(want_pose)))
                assert (got.iterations, got.termination, got.n_rows, got.used_mask) == (want["iterations"], want["termination"], want["n_rows"], want["used_mask"])
            if not kw:
                err = L.pose_error(want_pose, poses[6])
                assert want["termination"] == capi.LOCALIZE_CONVERGED and err[0] < 0.04 and err[1] < 0.03, err
        with pytest.raises((RuntimeError, TypeError)):
            m.localize(np.zeros((5, 2)), pose3d(poses[6]))
        with pytest.raises(RuntimeError):
            bad = loam.LocalizeParams()
            bad.neighborhood = 3
            m.localize(scans[6], pose3d(poses[6]), bad)
    finally:
        loc.close()
        cm.close()


@pytest.mark.gpu
def test_the_example_places_the_second_lap_on_the_map_of_the_first():
    _loam()
    spec = importlib.util.spec_from_file_location("localize_example", os.path.join(ROOT, "examples", "localize.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    out = example.main(scan_lines=16, points_per_line=256, verbose=False)
    n = len(out["after"])
    assert n == example.N_SECOND_LAP and len(out["before"]) == n and len(out["smallest_eigenvalue"]) == n
    assert np.median(out["after"]) < 0.25 * np.median(out["before"]) and max(out["after"]) < 0.1
    assert (np.asarray(out["termination"]) == capi.LOCALIZE_CONVERGED).all() and min(out["smallest_eigenvalue"]) > 0.0
