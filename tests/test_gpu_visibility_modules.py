"""The map cleaning through the layers above the C ABI: the pybind module `loam` (VisibilityParams, visibilityVotes,
removeDynamicPoints) and the C++ header shim (tests/cpp/test_visibility_shim.cpp, built with g++ and run as a child process) return
the C ABI's bytes on the same small input; the defaults are the C ABI's in all three layers; examples/clean_map.py removes the
moving box and keeps the rest, and its votes are the numpy model's on the scans and poses the example used."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import outdoor_scenes as S
import visibility_common as V
from loam_amd import build as B
from loam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _loam():
    B.build_pybind()
    if B.PY_DIR not in sys.path:
        sys.path.insert(0, B.PY_DIR)
    import loam
    return loam


def build_visibility_shim_test():
    B.build()
    exe = os.path.join(ROOT, "tests", "cpp", "test_visibility_shim")
    src = os.path.join(ROOT, "tests", "cpp", "test_visibility_shim.cpp")
    cmd = ["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", B.LIB_DIR, "-lloamx",
           "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{B.LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def test_visibility_shim_compiles_without_gpu():
    build_visibility_shim_test()


def test_python_module_exports_the_map_cleaning_api_with_the_c_abis_defaults_without_gpu():
    loam = _loam()
    assert callable(loam.visibilityVotes) and callable(loam.removeDynamicPoints)
    p, d, m = loam.VisibilityParams(), capi.VisibilityParams(), V.Params()
    st = capi.VisibilityParamsStruct()
    capi.load().loamx_default_visibility_params(st)
    for name in capi.VisibilityParams.FIELDS:
        assert getattr(p, name) == getattr(d, name) == getattr(st, name) == getattr(m, name), name
    assert set(capi.VisibilityParams.FIELDS) == set(V.Params.DEFAULTS)
    p.window_lines, p.through_ratio = 3, 0.5
    assert (p.window_lines, p.through_ratio) == (3, 0.5)
    assert capi.VISIBILITY_VOTES_DTYPE == V.VOTES_DTYPE and capi.VISIBILITY_VOTES_DTYPE.itemsize == 16
    assert capi.VISIBILITY_SCAN_CHUNK == V.SCAN_CHUNK
    for name in ("visibility_votes_dev", "visibility_votes", "visibility_filter_dev", "last_visibility_census"):
        assert callable(getattr(capi.Context, name))
    with pytest.raises(TypeError):
        capi.VisibilityParams(window=1)
    with pytest.raises(ValueError):
        capi.VisibilityParams(min_through=-1).struct()


@pytest.mark.gpu
def test_map_cleaning_through_cpp_shim():
    exe = build_visibility_shim_test()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:]
    assert " 0 failures" in out.stdout


@pytest.mark.gpu
def test_map_cleaning_through_the_python_module():
    from gpu_common import ctx
    loam = _loam()
    H, W = 16, 256
    lidar = loam.LidarParams(H, W, 1.0, 120.0)
    op = loam.OrganizeParams()
    op.elevations = V.O.fan_elevations(H, S.FANS["lot"])
    layout = loam.ScanLayout(lidar, op)
    clayout = ctx().scan_layout(capi.LidarParams(H, W, 1.0, 120.0), capi.OrganizeParams(elevations=V.O.fan_elevations(H, S.FANS["lot"])))
    try:
        d = V.drive()
        scans, poses7, pts = d["scans"][:6], d["poses"][:6], d["points"][:5000]
        poses = [loam.Pose3d(loam.Quaterniond(p[3], p[0], p[1], p[2]), p[4:]) for p in poses7]
        back = np.array([[q.rotation.x(), q.rotation.y(), q.rotation.z(), q.rotation.w(), *q.translation] for q in poses])
        for wl, ratio in ((1, 1.0), (0, 0.5)):
            p, cp = loam.VisibilityParams(), capi.VisibilityParams(window_lines=wl, through_ratio=ratio)
            p.window_lines, p.through_ratio = wl, ratio
            for sc in (scans, scans.astype(np.float64)):
                votes = loam.visibilityVotes(pts, sc, poses, layout, p)
                want = ctx().visibility_votes(pts, sc, back, clayout, cp)
                assert votes.dtype == np.uint32 and votes.shape == (len(pts), 4)
                assert V.same_bytes(votes.reshape(-1), want.view(np.uint32))
                assert want["agree"].sum() > len(pts) and want["through"].sum() > 0
            dynamic, index, kept = loam.removeDynamicPoints(pts, votes, p)
            m_dyn, m_xyz, m_keep, m_n = V.filter_static(want, V.Params(window_lines=wl, through_ratio=ratio), pts)
            assert dynamic.dtype == np.uint8 and index.dtype == np.uint32 and kept.dtype == np.float64
            assert V.same_bytes(dynamic, m_dyn) and V.same_bytes(index, m_keep) and V.same_bytes(kept, m_xyz) and 0 < m_n < len(pts)
        wide = np.concatenate([pts, np.ones((len(pts), 1))], axis=1)
        assert V.same_bytes(loam.visibilityVotes(wide, scans, poses, layout, p), votes)
        assert loam.visibilityVotes(pts[:0], scans, poses, layout).shape == (0, 4)
        assert len(loam.removeDynamicPoints(pts[:0], votes[:0])[0]) == 0
        with pytest.raises((RuntimeError, TypeError)):
            loam.visibilityVotes(pts, scans, poses[:2], layout)
        with pytest.raises(RuntimeError):
            loam.removeDynamicPoints(pts, votes[:5])
        with pytest.raises(RuntimeError):
            bad = loam.VisibilityParams()
            bad.window_cols = 4
            loam.visibilityVotes(pts, scans, poses, layout, bad)
    finally:
        clayout.close()


@pytest.mark.gpu
def test_the_example_removes_the_moving_box_and_its_votes_are_the_models():
    from gpu_common import ctx
    spec = importlib.util.spec_from_file_location("clean_map_example", os.path.join(ROOT, "examples", "clean_map.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    H, W = 16, 256
    out = example.main(scan_lines=H, points_per_line=W, leaf=0.4, verbose=False, ctx=ctx())
    layout = ctx().scan_layout(capi.LidarParams(H, W, 1.0, 120.0), capi.OrganizeParams(elevations=out["elevations"]))
    try:
        col, tan = layout.tables()
    finally:
        layout.close()
    votes, in_range, projected = V.votes(out["points"], out["scans"], out["poses"], H, W, col, tan)
    assert V.same_bytes(out["votes"], votes) and out["census"][2:] == (in_range, projected)
    dyn, xyz, _, n = V.filter_static(votes, None, out["points"])
    assert V.same_bytes(out["dynamic"].astype(np.uint8), dyn) and V.same_bytes(out["static"], xyz)
    box, rest = out["is_box"], out["is_rest"]
    # (the bounds of tests/test_visibility_model.py; the model alone gives 282 of 296 and 7 of 15 972 on this drive)
    assert box.sum() > 200 and (out["dynamic"] & box).sum() >= 0.9 * box.sum()
    assert rest.sum() > 10_000 and (out["dynamic"] & rest).sum() <= 0.005 * rest.sum()
