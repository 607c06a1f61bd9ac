"""CPU-only: map_math.h — the voxel key, the hash and the box test of the map upkeep kernels (loam_amd/csrc/map_kernels.hip)
— compiled with g++ (tests/hostcheck_map) against numpy. The GPU tests (test_gpu_voxel_filter.py, test_gpu_map_upkeep.py)
compare the kernels with the same numpy model."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "hostcheck_map")
BIAS = 1 << 20
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", DIR])
        _lib = C.CDLL(os.path.join(DIR, "libhostcheck_map.so"))
    return _lib


def header_keys(pts, leaf):
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    keys, ok = np.zeros(len(pts), dtype=np.uint64), np.zeros(len(pts), dtype=np.uint8)
    lib().hostcheck_map_keys(pts.ctypes.data_as(C.POINTER(C.c_double)), C.c_uint64(len(pts)), C.c_double(leaf),
                             keys.ctypes.data_as(C.POINTER(C.c_uint64)), ok.ctypes.data_as(C.POINTER(C.c_uint8)))
    return keys, ok.astype(bool)


def numpy_keys(pts, leaf):
    """the model of the issue: pack(np.floor(p / leaf)); ok = finite and |v| < 2^20 on every axis"""
    with np.errstate(all="ignore"):
        v = np.floor(np.asarray(pts, dtype=np.float64).reshape(-1, 3) / leaf)
    ok = np.all(np.abs(v) < BIAS, axis=1)  # (NaN compares false)
    b = np.where(ok[:, None], v, 0.0).astype(np.int64) + BIAS
    return ((b[:, 0] << 42) | (b[:, 1] << 21) | b[:, 2]).astype(np.uint64), ok


def test_keys_equal_numpy_on_random_points_lattices_zeros_and_the_range_edge():
    rng = np.random.default_rng(3)
    lattice = np.arange(-50, 50) * 0.4  # exact multiples of the leaf as numpy computes them: quotients on both sides of the integers
    q = lattice / 0.4
    assert (q < np.round(q)).any() and (q == np.round(q)).any(), "the lattice no longer straddles the integers"
    for leaf in (0.4, 0.2, 0.1, 1.0, 3.7):
        edge = BIAS * leaf
        special = np.array([[0.0, -0.0, 0.0], [-0.0, -0.0, -0.0], [edge, 0, 0], [-edge, 0, 0], [np.nextafter(edge, 0), 0, 0],
                            [np.nextafter(-edge, 0), 0, 0], [0, np.nextafter(edge, np.inf), 0], [0, 0, -edge - leaf],
                            [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e9, 0, 0], [1e300, -1e300, 0]])
        lat = np.arange(-50, 50) * leaf
        pts = np.concatenate([rng.uniform(-100, 100, (100_000, 3)), -np.abs(rng.normal(size=(1000, 3))) * 30,
                              np.stack(np.meshgrid(lat[::7], lat[::5], lat[::9], indexing="ij"), -1).reshape(-1, 3),
                              np.stack([lat, -lat, lat[::-1]], 1), special])
        got, got_ok = header_keys(pts, leaf)
        want, want_ok = numpy_keys(pts, leaf)
        assert np.array_equal(got_ok, want_ok), leaf
        assert np.array_equal(got[want_ok], want[want_ok]), leaf
        assert not got_ok[-5:].any() and got_ok[len(pts) - len(special)] and got_ok[len(pts) - len(special) + 4]
        assert (got[got_ok] != np.uint64(0xFFFFFFFFFFFFFFFF)).all()  # the empty mark is no key
    # -0.0 and +0.0 share a voxel; the range edge itself is outside, the value before it inside
    k, ok = header_keys([[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0]], 0.4)
    assert ok.all() and k[0] == k[1] == np.uint64((BIAS << 42) | (BIAS << 21) | BIAS)


def test_hash_stays_inside_the_table_for_every_capacity():
    rng = np.random.default_rng(4)
    keys, ok = header_keys(rng.uniform(-400, 400, (200_000, 3)), 0.1)
    keys = np.concatenate([keys[ok], np.array([0, 1, (1 << 63) - 1, ((2 * BIAS - 1) << 42) | ((2 * BIAS - 1) << 21) | (2 * BIAS - 1)], dtype=np.uint64)])
    for log2_cap in range(4, 25):
        mx, acc = C.c_uint32(0), C.c_uint32(0)
        lib().hostcheck_map_hash_range(keys.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_uint64(len(keys)), C.c_uint32(log2_cap),
                                       C.byref(mx), C.byref(acc))
        assert mx.value < (1 << log2_cap), log2_cap
        assert acc.value == (1 << log2_cap) - 1, log2_cap  # every bit of the slot index is in use
        want = ((keys * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(64 - log2_cap)).astype(np.uint32)  # (uint64 arithmetic wraps)
        assert mx.value == want.max()


def test_box_and_identity():
    rng = np.random.default_rng(5)
    pts = rng.uniform(-3, 3, (5000, 3))
    pts[:6] = [[1, 0, 0], [-1, 0, 0], [0, 2, 0], [0, -2, 0], [np.nan, 0, 0], [0, 0, np.inf]]
    lo, hi = np.array([-1.0, -2.0, -np.inf]), np.array([1.0, 2.0, 0.5])
    inside = np.zeros(len(pts), dtype=np.uint8)
    dp = C.POINTER(C.c_double)
    lib().hostcheck_map_box(pts.ctypes.data_as(dp), C.c_uint64(len(pts)), lo.ctypes.data_as(dp), hi.ctypes.data_as(dp),
                            inside.ctypes.data_as(C.POINTER(C.c_uint8)))
    with np.errstate(invalid="ignore"):
        want = np.all((pts >= lo) & (pts <= hi), axis=1)
    assert np.array_equal(inside.astype(bool), want) and want[:4].all() and not want[4:6].any()
    ident = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64)
    assert lib().hostcheck_map_pose_is_identity(ident.ctypes.data_as(dp)) == 1
    for i in range(7):
        p = ident.copy()
        p[i] += 1e-16 if i != 3 else -1e-15
        assert lib().hostcheck_map_pose_is_identity(p.ctypes.data_as(dp)) == 0, i
    neg = ident.copy()
    neg[0] = -0.0  # (a negative zero is still the identity: nothing is computed with it)
    assert lib().hostcheck_map_pose_is_identity(neg.ctypes.data_as(dp)) == 1


def test_pose_act_is_the_oracles(oracle):
    rng = np.random.default_rng(6)
    pts = rng.uniform(-50, 50, (2000, 3))
    q = rng.normal(size=4)
    pose = np.concatenate([q / np.linalg.norm(q), rng.uniform(-5, 5, 3)])
    out = np.zeros_like(pts)
    dp = C.POINTER(C.c_double)
    lib().hostcheck_map_pose_act(pose.ctypes.data_as(dp), pts.ctypes.data_as(dp), C.c_uint64(len(pts)), out.ctypes.data_as(dp))
    want = np.stack([oracle.pose_act(pose, p) for p in pts])
    assert np.abs(out - want).max() <= 1e-12 * (1 + np.abs(pts).max())


def test_the_same_functions_are_clean_under_asan_and_ubsan_in_a_stand_alone_program():
    subprocess.check_call(["make", "-s", "-C", DIR, "san"])
    out = subprocess.run([os.path.join(DIR, "hostcheck_map_san")], capture_output=True, text=True, timeout=300)
    text = out.stdout + out.stderr
    assert out.returncode == 0 and "hostcheck_map ok" in out.stdout, text[-3000:]
    assert "runtime error" not in text and "AddressSanitizer" not in text, text[-3000:]
