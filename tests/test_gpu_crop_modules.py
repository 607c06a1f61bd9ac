"""The map window through the layers above the C ABI, on the clouds, the centre and the boxes of the model comparison of
tests/test_gpu_crop.py (crop_common.case3_clouds): the C++ header shim (tests/cpp/test_crop_shim.cpp, built with g++ and run as a
child process on a file of those inputs) and the pybind module `loam` (CloudMap.crop, SurfelMap.crop, OccupancyMap.crop) return
the bytes of the ctypes layer, which tests/test_gpu_crop.py compares with the models."""
import importlib.util
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import cloudmap_common as CM
import crop_common as X
from loam_amd import build as B
from loam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAF, MAX_VOXELS = 0.5, 4096
BOX_VMIN, BOX_DIMS = [-14, -14, -6], [34, 28, 12]


def _loam():
    B.build_pybind()
    if B.PY_DIR not in sys.path:
        sys.path.insert(0, B.PY_DIR)
    import loam
    return loam


def build_crop_shim_test():
    B.build()
    exe = os.path.join(ROOT, "tests", "cpp", "test_crop_shim")
    src = os.path.join(ROOT, "tests", "cpp", "test_crop_shim.cpp")
    cmd = ["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", B.LIB_DIR, "-lloamx",
           "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{B.LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def inputs():
    """the three clouds, the fourth, and which clouds are in the map before each box"""
    (pts, off, poses), (pts4, off4, poses4) = X.case3_clouds()
    return (np.concatenate([pts, pts4]), np.concatenate([off, off4[1:] + off[-1]]), np.concatenate([poses, poses4]), [len(poses), len(poses) + 1])


def test_crop_shim_compiles_without_gpu():
    build_crop_shim_test()


def test_the_layers_export_the_crop_without_gpu():
    loam = _loam()
    for cls in (loam.CloudMap, loam.SurfelMap, loam.OccupancyMap, capi.CloudMap, capi.SurfelMap, capi.OccupancyMap):
        assert callable(getattr(cls, "crop"))
    for cls in (capi.CloudMap, capi.SurfelMap, capi.OccupancyMap):
        assert callable(getattr(cls, "crop_dev"))
    lib = capi.load()
    for name in ("loamx_cloud_map_crop", "loamx_surfel_map_crop", "loamx_occupancy_crop"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert capi.K_COUNT == 15  # (the crop runs untimed: no scope of its own)
    with pytest.raises(ValueError):
        capi._VoxelMap._crop_bounds([0.0, 0.0], [1.0, 1.0, 1.0], "crop")
    with pytest.raises(ValueError):
        capi._VoxelMap._crop_bounds([0.0, 0.0, 0.0], ["a", "b", "c"], "crop")


@pytest.mark.gpu
def test_crop_through_cpp_shim():
    exe = build_crop_shim_test()
    pts, off, poses, before = inputs()
    head = [len(poses), len(pts), LEAF, MAX_VOXELS, *X.CASE3_CENTRE, len(X.CASE3_BOXES)]
    for lo, hi in X.CASE3_BOXES:
        head += [*lo, *hi]
    blob = np.concatenate([np.array(head + before, dtype=np.float64), off.astype(np.float64), poses.reshape(-1), pts.reshape(-1)])
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "crop_inputs.bin")
        blob.tofile(path)
        out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:]
    assert " 0 failures" in out.stdout


@pytest.mark.gpu
def test_crop_through_the_python_module():
    from gpu_common import ctx
    loam = _loam()
    pts, off, poses, before = inputs()
    c = ctx()
    params = []
    for cls in (loam.CloudMapParams, loam.SurfelMapParams, loam.OccupancyParams):
        p = cls()
        p.leaf, p.min_range, p.max_range = LEAF, 0.01, 80.0
        params.append(p)
    mods = [loam.CloudMap(params[0], MAX_VOXELS), loam.SurfelMap(params[1], MAX_VOXELS), loam.OccupancyMap(params[2], MAX_VOXELS)]
    caps = [c.cloud_map(capi.CloudMapParams(LEAF, 0.01, 80.0), MAX_VOXELS), c.surfel_map(capi.SurfelMapParams(LEAF, 0.01, 80.0), MAX_VOXELS),
            c.occupancy_map(capi.OccupancyParams(leaf=LEAF, min_range=0.01, max_range=80.0), MAX_VOXELS)]

    def compare(what):
        xyz, counts, first = mods[0].points()
        CM.assert_emit_equal((xyz, counts, first, len(counts)), caps[0].emit(), what)
        got, (want, n) = mods[1].surfels(), caps[1].emit()
        assert len(got["count"]) == n
        for name in ("mean", "cov", "eval", "normal", "count", "first"):
            assert CM.same_bytes(got[name], np.ascontiguousarray(want[name])), (what, name)
        got, want = mods[2].box(BOX_VMIN, BOX_DIMS), caps[2].box(np.array(BOX_VMIN), np.array(BOX_DIMS))
        assert CM.same_bytes(got[0], want[0]) and CM.same_bytes(got[1], want[1]), what
        for mod, cap in zip(mods, caps):
            st, want_st = mod.stats(), cap.stats()
            assert int(st["voxels"]) == int(want_st["voxels"]) and int(st["overflow"]) == 0, what

    try:
        added = 0
        for b, (lo, hi) in enumerate(X.CASE3_BOXES):
            for i in range(added, before[b]):
                p7 = poses[i]
                pose = loam.Pose3d(loam.Quaterniond(p7[3], p7[0], p7[1], p7[2]), p7[4:])
                back = np.array([pose.rotation.x(), pose.rotation.y(), pose.rotation.z(), pose.rotation.w(), *pose.translation])
                for mod, cap in zip(mods, caps):
                    mod.add(pts[off[i]:off[i + 1]], pose)
                    cap.add_cloud(pts[off[i]:off[i + 1]], back)
            added = before[b]
            compare(f"before box {b}")
            for mod, cap in zip(mods, caps):
                got = mod.crop(lo, hi, list(X.CASE3_CENTRE))
                assert tuple(got) == cap.crop(lo, hi, X.CASE3_CENTRE) and got[0] > 50 and got[1] > 50, (b, got)
            compare(f"after box {b}")
        assert tuple(mods[0].crop([-1e9] * 3, [1e9] * 3)) == (int(caps[0].stats()["voxels"]), 0)  # the default centre
        with pytest.raises(RuntimeError):
            mods[1].crop([1.0, 0.0, 0.0], [0.0, 1.0, 1.0])
        with pytest.raises(RuntimeError):
            mods[2].crop([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [np.nan, 0.0, 0.0])
        with pytest.raises(TypeError):
            mods[0].crop([0.0, 0.0], [1.0, 1.0, 1.0])
        compare("after the refusals")
    finally:
        for cap in caps:
            cap.close()


@pytest.mark.gpu
def test_the_example_follows_the_sensor_with_a_map_that_an_uncropped_drive_overflows():
    spec = importlib.util.spec_from_file_location("sliding_map_example", os.path.join(ROOT, "examples", "sliding_map.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    n = 60
    out = example.main(n_scans=n, verbose=False)
    assert len(out["voxels"]) == len(out["removed"]) == n - example.N_SEED and out["skipped"] == 0
    assert out["overflow"] == 0 and out["final_voxels"] == out["voxels"][-1]
    assert max(k + r for k, r in zip(out["voxels"], out["removed"])) <= out["max_voxels"] == 8192  # (the map before each crop fitted)
    assert min(out["removed"]) > 0  # (every crop had something to remove)
    assert out["uncropped_overflow"] > 0 and out["uncropped_voxels"] == out["max_voxels"]  # the same drive without a crop does not fit
    assert max(out["error"]) < 1.0  # (the drive stayed on the street: the window is 15 m)
