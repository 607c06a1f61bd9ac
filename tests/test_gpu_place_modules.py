"""Place recognition through the layers above the C ABI: the pybind module `loam` (PlaceParams, PlaceMatch, PlaceDatabase) and the
C++ header shim (tests/cpp/test_place_shim.cpp, built with g++ and run as a child process) return the C ABI's bytes on the same
scans; the defaults are the C ABI's in all three layers; examples/loop_closure.py closes its loop."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

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


def build_place_shim_test():
    B.build()
    exe = os.path.join(ROOT, "tests", "cpp", "test_place_shim")
    src = os.path.join(ROOT, "tests", "cpp", "test_place_shim.cpp")
    cmd = ["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", B.LIB_DIR, "-lloamx",
           "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{B.LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def test_place_shim_compiles_without_gpu():
    build_place_shim_test()


def test_python_module_exports_the_place_api_with_the_c_abis_defaults_without_gpu():
    loam = _loam()
    assert hasattr(loam, "PlaceDatabase") and hasattr(loam, "PlaceMatch")
    for name in ("descriptor", "add", "search", "size"):
        assert callable(getattr(loam.PlaceDatabase, name))
    assert callable(loam.PlaceMatch.initialGuess)
    p, d = loam.PlaceParams(), capi.PlaceParams()
    st = capi.PlaceParamsStruct()
    capi.load().loamx_default_place_params(st)
    want = (20, 60, 80.0, 2.0, 64.0)
    assert (p.n_rings, p.n_sectors, p.max_range, p.z_offset, p.z_scale) == want
    assert (d.n_rings, d.n_sectors, d.max_range, d.z_offset, d.z_scale) == want
    assert (st.n_rings, st.n_sectors, st.max_range, st.z_offset, st.z_scale) == want
    p.n_rings, p.z_scale = 4, 32.0
    assert (p.n_rings, p.z_scale) == (4, 32.0)
    assert capi.PLACE_MATCH_DTYPE.itemsize == 24
    for name in ("descriptors_dev", "descriptor", "add", "add_dev", "size", "read", "search", "search_dev", "sector_dirs", "close"):
        assert callable(getattr(capi.PlaceDb, name))
    assert callable(capi.Context.place_db)


@pytest.mark.gpu
def test_place_through_cpp_shim():
    exe = build_place_shim_test()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:]
    assert " 0 failures" in out.stdout


@pytest.mark.gpu
def test_place_through_the_python_module():
    from gpu_common import ctx
    loam = _loam()
    H, W = 16, 256
    p = loam.PlaceParams()
    p.n_rings, p.n_sectors, p.max_range = 12, 40, 60.0
    db = loam.PlaceDatabase(p)
    cdb = ctx().place_db(capi.PlaceParams(12, 40, 60.0))
    try:
        assert np.array_equal(db.sectorDirections(), cdb.sector_dirs())
        assert (db.params.n_rings, db.params.n_sectors, db.size(), len(db)) == (12, 40, 0, 0)
        descs = []
        for i, name in enumerate(S.SCENES):
            o, yaw = S.sensor_origin(name, 0)
            scan = S.scan_at(name, 0, o, yaw, H, W, noise_seed=1)
            for cloud in (scan, scan.astype(np.float32), np.concatenate([scan, np.ones((len(scan), 1))], axis=1)):
                got = db.descriptor(cloud)
                assert got.dtype == np.uint16 and got.shape == (12, 40) and np.array_equal(got, cdb.descriptor(cloud))
            d = db.descriptor(scan)
            assert db.add(d) == i == cdb.add(d)
            descs.append(d)
        assert db.size() == 3 == cdb.size()
        o, yaw = S.sensor_origin("lot", 0)
        q = db.descriptor(S.scan_at("lot", 0, o, yaw + 9 * 2 * np.pi / 40, H, W, noise_seed=2))
        for id_end in (None, 3, 1, 0):
            got = db.search(q, 3, id_end)
            want = cdb.search(q, 3, id_end)[0]
            assert [m.id for m in got] == want["id"].tolist() and [m.shift for m in got] == want["shift"].tolist()
            assert [m.key_dist for m in got] == want["key_dist"].tolist()
            assert np.array([m.distance for m in got]).tobytes() == want["distance"].tobytes()
            assert [m.valid for m in got] == (want["id"] != capi.PLACE_NO_ID).tolist()
        best = db.search(q, 3)[0]
        assert (best.id, best.shift) == (1, 9) and best.yaw == 2 * np.pi * 9 / 40
        g = best.initialGuess()
        assert abs(g.rotation.z() - np.sin(best.yaw / 2)) < 1e-15 and abs(g.rotation.w() - np.cos(best.yaw / 2)) < 1e-15
        assert (g.rotation.x(), g.rotation.y(), g.translation[0], g.translation[1], g.translation[2]) == (0.0, 0.0, 0.0, 0.0, 0.0)
        with pytest.raises(RuntimeError):
            db.search(q[:3], 3)
        with pytest.raises(RuntimeError):
            db.search(q, 65)
        with pytest.raises((RuntimeError, TypeError)):
            db.descriptor(np.zeros((5, 2)))
        with pytest.raises(RuntimeError):
            bad = loam.PlaceParams()
            bad.n_sectors = 2
            loam.PlaceDatabase(bad)
    finally:
        cdb.close()


@pytest.mark.gpu
def test_the_example_closes_its_loop():
    _loam()
    spec = importlib.util.spec_from_file_location("loop_closure_example", os.path.join(ROOT, "examples", "loop_closure.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    loops = example.main(verbose=False)
    assert len(loops) >= 1
    for lp in loops:
        assert lp["query"] - lp["entry"] >= example.MIN_AGE
        assert lp["rotation_error"] < np.radians(1.0) and lp["translation_error"] < 0.1, lp
    assert any(lp["query"] == example.N_SCANS - 1 and lp["entry"] == 0 for lp in loops)  # the drive ends where it began
