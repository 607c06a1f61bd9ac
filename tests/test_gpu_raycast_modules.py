"""The occupancy ray cast through the layers above the C ABI: the C++ header shim (tests/cpp/test_raycast_shim.cpp, built with g++
and run as a child process) and the pybind module `loam` (OccupancyMap.castRays / renderScans) return the bytes of the ctypes
layer, which tests/test_gpu_raycast.py compares with the model; the defaults are the C ABI's in all three layers; and the cells of
capi.beam_directions organise back into their own cell."""
import os
import subprocess
import sys

import numpy as np
import pytest

import raycast_common as M
from loam_amd import build as B
from loam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _loam():
    B.build_pybind()
    if B.PY_DIR not in sys.path:
        sys.path.insert(0, B.PY_DIR)
    import loam
    return loam


def build_raycast_shim_test():
    B.build()
    exe = os.path.join(ROOT, "tests", "cpp", "test_raycast_shim")
    src = os.path.join(ROOT, "tests", "cpp", "test_raycast_shim.cpp")
    cmd = ["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", B.LIB_DIR, "-lloamx",
           "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{B.LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def test_raycast_shim_compiles_without_gpu():
    build_raycast_shim_test()


def test_the_layers_export_the_ray_cast_without_gpu():
    loam = _loam()
    for name in ("castRays", "renderScans"):
        assert callable(getattr(loam.OccupancyMap, name))
    for name in ("cast_rays_dev", "cast_rays", "render_scans_dev", "render_scans"):
        assert callable(getattr(capi.OccupancyMap, name))
    assert callable(capi.Context.last_raycast_census)
    lib = capi.load()
    for name in ("loamx_default_raycast_params", "loamx_occupancy_cast_rays", "loamx_occupancy_render_scans", "loamx_occupancy_cast_rays_host",
                 "loamx_occupancy_render_scans_host", "loamx_ctx_last_raycast_census"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    p, q = loam.RaycastParams(), capi.RaycastParams()
    assert (p.skip_start, bool(p.unknown_stops), p.max_steps, p.hit_at) == (q.skip_start, bool(q.unknown_stops), q.max_steps, q.hit_at)
    assert (q.skip_start, q.unknown_stops, q.max_steps, q.hit_at) == tuple(M.DEFAULTS[k] for k in ("skip_start", "unknown_stops", "max_steps", "hit_at"))
    assert capi.RAY_RECORD_DTYPE == M.RECORD_DTYPE and capi.RAYCAST_CENSUS_DTYPE.names == M.CENSUS_NAMES
    assert (capi.RAY_CLEAR, capi.RAY_HIT, capi.RAY_UNKNOWN, capi.RAY_TRUNCATED, capi.RAY_OUTSIDE, capi.RAY_INVALID) == tuple(range(6))
    assert [getattr(loam.OccupancyMap, "RAY_" + n.upper()) for n in M.STATUS_NAMES] == list(range(6))
    assert (loam.OccupancyMap.RAY_AT_ENTER, loam.OccupancyMap.RAY_AT_MIDDLE) == (capi.RAY_AT_ENTER, capi.RAY_AT_MIDDLE) == (M.AT_ENTER, M.AT_MIDDLE)
    with pytest.raises(ValueError):
        capi.RaycastParams(max_steps=-1).struct()


def test_beam_directions_are_the_unit_centres_of_the_cells_without_gpu():
    o = capi.OrganizeParams(azimuth_zero=0.3, clockwise=True, elevations=np.radians([-10.0, -2.0, 1.0]))
    d = capi.beam_directions(3, 8, o).reshape(3, 8, 3)
    assert np.allclose(np.linalg.norm(d, axis=2), 1.0, atol=1e-15)
    assert np.allclose(np.arcsin(d[:, :, 2]), np.radians([-10.0, -2.0, 1.0])[:, None])
    az = np.arctan2(d[0, :, 1], d[0, :, 0])
    assert np.allclose(np.angle(np.exp(1j * (az - (0.3 - 2 * np.pi * np.arange(8) / 8)))), 0.0, atol=1e-12)
    lin = capi.beam_directions(4, 6, capi.OrganizeParams(fov_bottom=-0.3, fov_top=0.3)).reshape(4, 6, 3)
    assert np.allclose(np.arcsin(lin[:, 0, 2]), [-0.3, -0.1, 0.1, 0.3])
    with pytest.raises(ValueError):
        capi.beam_directions(4, 8, o)


@pytest.mark.gpu
def test_raycast_through_cpp_shim():
    exe = build_raycast_shim_test()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:]
    assert " 0 failures" in out.stdout


@pytest.mark.gpu
def test_raycast_through_the_python_module():
    from gpu_common import ctx
    loam = _loam()
    model, cloud, pose7 = M.room_model()
    p = loam.OccupancyParams()
    p.leaf, p.min_range, p.max_range, p.end_margin = (model.p[k] for k in ("leaf", "min_range", "max_range", "end_margin"))
    mod = loam.OccupancyMap(p, 1 << 17)
    cap = ctx().occupancy_map(capi.OccupancyParams(**{k: model.p[k] for k in ("leaf", "min_range", "max_range", "end_margin")}), 1 << 17)
    try:
        pose = loam.Pose3d(loam.Quaterniond(pose7[3], pose7[0], pose7[1], pose7[2]), pose7[4:])
        mod.add(cloud, pose)
        cap.add_cloud(cloud, pose7)
        states = M.StateMap.of(model)
        rng = np.random.default_rng(4)
        o, e = rng.uniform(-2.0, 2.0, (70, 3)) * [1.0, 1.0, 0.5], rng.uniform(-6.0, 6.0, (70, 3))
        for kw in ({}, dict(unknown_stops=1, skip_start=2), dict(max_steps=4)):
            rp = loam.RaycastParams()
            for k, v in kw.items():
                setattr(rp, k, v)
            got, want, ref = mod.castRays(o, e, rp), cap.cast_rays(o, e, capi.RaycastParams(**kw)), M.cast(o, e, model.p["leaf"], states, kw)[0]
            assert got.dtype == want.dtype == M.RECORD_DTYPE and M.same_bytes(got, want) and M.same_bytes(got, ref), kw
        assert (ref["status"] == M.TRUNCATED).any()
        dirs = capi.beam_directions(3, 70)
        poses = np.stack([pose7, np.array([0.0, 0.0, np.sin(0.4), np.cos(0.4), 0.5, -0.3, 0.1])])
        for hit_at in (M.AT_ENTER, M.AT_MIDDLE):
            rp = loam.RaycastParams()
            rp.hit_at = hit_at
            got, want = mod.renderScans(dirs, poses, 9.0, rp), cap.render_scans(dirs, poses, 9.0, capi.RaycastParams(hit_at=hit_at))
            ref = M.render(dirs, poses, 9.0, model.p["leaf"], states, dict(hit_at=hit_at))
            for g, w, r in zip(got, want, ref):
                assert g.shape == w.shape == r.shape and g.dtype == w.dtype and M.same_bytes(g, w) and M.same_bytes(g, r), hit_at
        assert (ref[2]["status"] == M.HIT).mean() > 0.9
        rp = loam.RaycastParams()
        rp.max_steps = (1 << 22) + 1
        with pytest.raises(RuntimeError):
            mod.castRays(o, e, rp)
        with pytest.raises(RuntimeError):
            mod.renderScans(dirs, poses, 0.0)
    finally:
        cap.close()


@pytest.mark.gpu
def test_the_rendered_scan_of_a_closed_room_organises_back_into_its_own_cells():
    from gpu_common import ctx
    c = ctx()
    model, cloud, pose7 = M.room_model()
    m = c.occupancy_map(capi.OccupancyParams(**{k: model.p[k] for k in ("leaf", "min_range", "max_range", "end_margin")}), 1 << 17)
    H, W = 4, 64
    o = capi.OrganizeParams(azimuth_zero=0.2, fov_bottom=np.radians(-20.0), fov_top=np.radians(15.0))
    layout = c.scan_layout(capi.LidarParams(H, W, 0.1, 120.0), o)
    try:
        m.add_cloud(cloud, pose7)
        scans, ranges, records = m.render_scans(capi.beam_directions(H, W, o), pose7[None], 9.0)
        assert (records["status"][0] == capi.RAY_HIT).mean() > 0.9 and (ranges[0] > 0.5).sum() > 0.9 * H * W
        scan, src, stats = c.organize_cloud(scans[0], layout)
        filled = scans[0].any(axis=1)
        assert (src[filled] == np.flatnonzero(filled)).all() and (src[~filled] == capi.NO_POINT).all()
        assert M.same_bytes(scan, scans[0]) and int(stats[0]) == int(filled.sum()) and int(stats[3]) == 0
    finally:
        layout.close(), m.close()
