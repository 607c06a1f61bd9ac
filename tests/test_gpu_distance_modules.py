"""The occupancy distance field through the layers above the C ABI: the C++ header shim (tests/cpp/test_distance_shim.cpp, built
with g++ and run as a child process) and the pybind module `loam` (OccupancyMap.distanceBox / distanceSlice) return the bytes of
the ctypes layer, which tests/test_gpu_distance.py compares with the model; the defaults are the C ABI's in all three layers; and
examples/clearance.py turns the slice of its drive into a clearance grid that equals the model's field of the slice it printed."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import distance_common as D
import occupancy_common as M
from loam_amd import build as B
from loam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _loam():
    B.build_pybind()
    if B.PY_DIR not in sys.path:
        sys.path.insert(0, B.PY_DIR)
    import loam
    return loam


def build_distance_shim_test():
    B.build()
    exe = os.path.join(ROOT, "tests", "cpp", "test_distance_shim")
    src = os.path.join(ROOT, "tests", "cpp", "test_distance_shim.cpp")
    cmd = ["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", B.LIB_DIR, "-lloamx",
           "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{B.LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def test_distance_shim_compiles_without_gpu():
    build_distance_shim_test()


def test_the_layers_export_the_distance_field_without_gpu():
    loam = _loam()
    for name in ("distanceBox", "distanceSlice"):
        assert callable(getattr(loam.OccupancyMap, name))
    for name in ("distance_box_dev", "distance_box", "distance_slice_dev", "distance_slice"):
        assert callable(getattr(capi.OccupancyMap, name))
    lib = capi.load()
    for name in ("loamx_default_distance_params", "loamx_occupancy_distance_box", "loamx_occupancy_distance_slice",
                 "loamx_occupancy_distance_box_host", "loamx_occupancy_distance_slice_host"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    p, q = loam.DistanceParams(), capi.DistanceParams()
    assert (p.max_dist_voxels, bool(p.unknown_is_obstacle)) == (q.max_dist_voxels, bool(q.unknown_is_obstacle)) == (10, False)
    assert loam.OccupancyMap.DIST_FAR == capi.DIST_FAR == D.FAR
    with pytest.raises(ValueError):
        capi.DistanceParams(max_dist_voxels=-1).struct()


@pytest.mark.gpu
def test_distance_through_cpp_shim():
    exe = build_distance_shim_test()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:]
    assert " 0 failures" in out.stdout


@pytest.mark.gpu
def test_distance_through_the_python_module():
    from gpu_common import ctx
    loam = _loam()
    pts, pose7 = M.random_rays(54, 1500, 5.0)  # the scene of the model comparison's host forms
    p = loam.OccupancyParams()
    p.leaf = 0.25
    mod = loam.OccupancyMap(p, 1 << 17)
    cap = ctx().occupancy_map(capi.OccupancyParams(leaf=0.25), 1 << 17)
    model = M.OccupancyModel(leaf=0.25)
    try:
        pose = loam.Pose3d(loam.Quaterniond(pose7[3], pose7[0], pose7[1], pose7[2]), pose7[4:])
        back = np.array([pose.rotation.x(), pose.rotation.y(), pose.rotation.z(), pose.rotation.w(), *pose.translation])
        mod.add(pts, pose)
        cap.add_cloud(pts, back)
        model.add(pts, poses=back[None])
        sensor = np.floor(back[4:] / 0.25).astype(np.int64)
        vmin, dims = (sensor - [6, 5, 2]).tolist(), [12, 10, 4]
        for unknown in (False, True):
            dp = loam.DistanceParams()
            dp.max_dist_voxels, dp.unknown_is_obstacle = 3, unknown
            cp = capi.DistanceParams(3, int(unknown))
            for got, want, ref in ((mod.distanceBox(vmin, dims, dp), cap.distance_box(vmin, dims, cp), D.model_field(model, vmin, dims, 3, unknown)),
                                   (mod.distanceSlice(vmin, dims, dp), cap.distance_slice(vmin, dims, cp), D.model_field(model, vmin, dims, 3, unknown, True))):
                for g, w, r in zip(got, want, ref):
                    assert g.shape == w.shape == r.shape and g.dtype == w.dtype and M.same_bytes(g, w) and M.same_bytes(g, r), unknown
        got, want = mod.distanceSlice(vmin, dims), cap.distance_slice(vmin, dims)  # the default parameters
        assert all(M.same_bytes(g, w) for g, w in zip(got, want)) and (got[0] == 0).any()
        dp = loam.DistanceParams()
        dp.max_dist_voxels = 0
        with pytest.raises(RuntimeError):
            mod.distanceBox(vmin, dims, dp)
        with pytest.raises(RuntimeError):
            mod.distanceBox([1 << 31, 0, 0], dims)
    finally:
        cap.close()


@pytest.mark.gpu
def test_the_example_prints_a_clearance_grid_that_is_the_field_of_its_slice():
    spec = importlib.util.spec_from_file_location("clearance_example", os.path.join(ROOT, "examples", "clearance.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    out = example.main(scan_lines=16, points_per_line=256, leaf=0.4, radius=0.9, verbose=False)
    grid, d2, R = out["slice"], out["d2"], out["max_dist_voxels"]
    assert R == 5 and all((grid == s).any() for s in (M.UNKNOWN, M.FREE, M.OCCUPIED))
    assert ((d2 == 0) == (grid == M.OCCUPIED)).all()
    # R cells inside the grid's edge no obstacle outside the grid can matter: there the field is the field of the printed slice
    h, w = grid.shape
    ys, xs = np.nonzero(grid == M.OCCUPIED)
    want = D.field(np.stack([xs, ys], axis=1), (R, R), (w - 2 * R, h - 2 * R), R, out["leaf"])
    inner = (slice(R, h - R), slice(R, w - R))
    assert M.same_bytes(d2[inner], want[0]) and M.same_bytes(out["offset"][inner], want[1]) and M.same_bytes(out["metres"][inner], want[2])
    free = grid == M.FREE
    tight = free & (out["metres"] < out["radius"])
    assert out["tight_cells"] == int(tight.sum()) and 0 < out["tight_cells"] < out["free_cells"] == int(free.sum())
    assert ((out["classes"] == 2) == tight).all() and 0.0 < out["tight_share"] < 0.5
    assert len(example.picture(out["classes"], 2).split("\n")) == h // 2
