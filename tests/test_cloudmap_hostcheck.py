"""CPU-only: cloudmap_math.h — validity, voxel and 32-bit offset, centroid of the cloud map kernels
(loam_amd/csrc/cloudmap_kernels.hip) — compiled with g++ (tests/hostcheck_cloudmap) against the numpy model of
tests/cloudmap_common.py, by equality. The GPU tests (test_gpu_cloudmap.py) compare the kernels with the same model."""
import ctypes as C
import os
import subprocess

import numpy as np

import cloudmap_common as M

dp, u64p, u32p = C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)


def header_cells(pts, leaf):
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    n = len(pts)
    keys, u, ok = np.zeros(n, dtype=np.uint64), np.zeros((n, 3), dtype=np.uint32), np.zeros(n, dtype=np.uint8)
    M.hostcheck_lib().hostcheck_cloudmap_cells(pts.ctypes.data_as(dp), C.c_uint64(n), C.c_double(leaf), keys.ctypes.data_as(u64p),
                                               u.ctypes.data_as(u32p), ok.ctypes.data_as(C.POINTER(C.c_uint8)))
    return keys, u, ok.astype(bool)


def header_validity(pts, min_range, max_range):
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    what = np.zeros(len(pts), dtype=np.int32)
    M.hostcheck_lib().hostcheck_cloudmap_validity(pts.ctypes.data_as(dp), C.c_uint64(len(pts)), C.c_double(min_range * min_range),
                                                  C.c_double(max_range * max_range), what.ctypes.data_as(C.POINTER(C.c_int32)))
    return what


def header_centroids(keys, sums, counts, leaf):
    keys, sums = np.ascontiguousarray(keys, dtype=np.uint64), np.ascontiguousarray(sums, dtype=np.uint64).reshape(-1, 3)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    out = np.zeros((len(keys), 3))
    M.hostcheck_lib().hostcheck_cloudmap_centroids(keys.ctypes.data_as(u64p), sums.ctypes.data_as(u64p), counts.ctypes.data_as(u32p),
                                                   C.c_uint64(len(keys)), C.c_double(leaf), out.ctypes.data_as(dp))
    return out


def test_the_model_equals_the_g_plus_plus_build_on_faces_the_clamp_the_range_edges_and_large_sums():
    rng = np.random.default_rng(11)
    saw_clamp = False
    for leaf in (0.4, 0.2, 0.1, 1.0, 3.7):
        lat = np.arange(-50, 50) * leaf  # points on voxel faces: quotients on both sides of the integers at leaf 0.4
        edge = M.BIAS * leaf
        special = np.array([[1e-20, -1e-20, 0.0], [-1e-20, -0.0, 1.0], [-0.0, -0.0, -0.0], [-5e-324, 5e-324, 3.0],
                            [(M.BIAS - 0.5) * leaf, 0, 0], [-(M.BIAS - 1.5) * leaf, 0, 0],                          # v = 2^20 - 1, -(2^20 - 1)
                            [-(M.BIAS - 0.5) * leaf, 0, 0], [edge, 0, 0], [0, np.nextafter(edge, np.inf), 0], [0, 0, -edge - leaf],  # |v| = 2^20 and beyond
                            [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e300, -1e300, 0],
                            [edge + 0.37 * leaf, 0.53 * leaf, -0.29 * leaf], [0.41 * leaf, np.nan, 7.77 * leaf]])  # out of range on one axis only
        pts = np.concatenate([rng.uniform(-100, 100, (50_000, 3)), -np.abs(rng.normal(size=(1000, 3))) * 30,
                              np.stack([lat, -lat, lat[::-1]], 1), special])
        keys, u, ok = header_cells(pts, leaf)
        m_ok, m_v, m_u = M.cells(pts, leaf)
        assert np.array_equal(ok, m_ok), leaf
        assert np.array_equal(keys[ok], M.pack(m_v)[ok]), leaf
        assert np.array_equal(u[ok].astype(np.uint64), m_u[ok]), leaf
        assert not u[~ok].any() and (~ok).sum() >= 8, leaf  # a point without a voxel carries no offsets, whatever its other axes say
        s = len(pts) - len(special)
        assert ok[s:s + 6].all() and not ok[s + 6:].any(), (leaf, ok[s:])
        assert (u[s + 0, 1], u[s + 1, 0]) == (M.U32_MAX, M.U32_MAX) and (u[s + 1, 1], u[s + 2, 0]) == (0, 0)  # -1e-20: frac == 1.0, clamped; -0.0: 0
        assert int(keys[s + 4] >> np.uint64(42)) == 2 * M.BIAS - 1 and int(keys[s + 5] >> np.uint64(42)) == 1
        saw_clamp |= bool((u[ok] == M.U32_MAX).any())
        if leaf == 0.4:
            q = (np.arange(-50, 50) * 0.4) / 0.4
            assert (q < np.round(q)).any() and (q == np.round(q)).any(), "the lattice no longer straddles the integers"
    assert saw_clamp

    # validity: both range edges from both sides, zeros, non-finite coordinates and a non-finite r2
    for lo, hi in ((0.5, 120.0), (0.0, 1.0), (2.0, 2.0)):
        r = np.array([lo, np.nextafter(lo, 0), np.nextafter(lo, np.inf), hi, np.nextafter(hi, 0), np.nextafter(hi, np.inf), 0.0, 1e200])
        pts = np.concatenate([np.stack([r, 0 * r, 0 * r], 1), np.stack([0 * r, -r, 0 * r], 1), rng.normal(size=(5000, 3)) * hi / 2,
                              [[np.nan, 0, 0], [0, -np.inf, 0], [1e155, 1e155, 0]]])
        assert np.array_equal(header_validity(pts, lo, hi), M.validity(pts, lo, hi)), (lo, hi)
    got = header_validity([[0, 0, 0], [0.5, 0, 0], [np.nextafter(0.5, 0), 0, 0], [1e200, 0, 0], [np.nan, 1, 1]], 0.5, 120.0)
    assert got.tolist() == [M.RANGE, M.USED, M.RANGE, M.INVALID, M.INVALID]

    # centroids: uint64 -> double of sums near 2^63 (a synthetic count: 2^31 points at the largest offset), small sums, odd counts
    counts = np.array([1, 2, 3, 7, 1000, 1 << 31, (1 << 32) - 2, 12345], dtype=np.uint32)
    sums = np.stack([counts.astype(np.uint64) * np.uint64(M.U32_MAX), counts.astype(np.uint64) * np.uint64(0x80000001),
                     counts.astype(np.uint64) * np.uint64(3) + np.uint64(1)], 1)
    assert int(sums.max()) > (1 << 63) - (1 << 33) and ((sums.astype(np.float64).astype(np.uint64) != sums).any()), "no sum needs rounding"
    v = rng.integers(-M.BIAS + 1, M.BIAS, (len(counts), 3))
    for leaf in (0.2, 0.4, 3.7):
        assert M.same_bytes(header_centroids(M.pack(v), sums, counts, leaf), M.centroid(v, sums, counts, leaf)), leaf


def test_the_model_map_keeps_order_of_first_appearance_and_counts_every_drop():
    m = M.CloudMapModel(1.0, 0.5, 10.0)
    pts = np.array([[2.5, 0, 0], [1.5, 0, 0], [2.25, 0, 0], [0, 0, 0], [np.nan, 0, 0], [11, 0, 0], [1.75, 0.5, 0]])
    m.add(pts)
    m.add(np.array([[3.5, 0, 0], [2.75, 0, 0]]), poses=np.array([[0, 0, 0, 1.0, 0, 0, 0]]))
    xyz, count, first, n = m.emit()
    assert n == 3 and first.tolist() == [0, 1, 7] and count.tolist() == [3, 2, 1]
    assert xyz.tolist() == [[2.5, 0.0, 0.0], [1.625, 0.25, 0.0], [3.5, 0.0, 0.0]]
    assert m.stats() == dict(voxels=3, points_offered=9, points_used=6, invalid=1, range=2, outside=0, overflow=0)
    assert m.emit(2)[3] == 2 and m.emit(1, capacity=1)[2].tolist() == [0]


def test_the_same_functions_are_clean_under_asan_and_ubsan_in_a_stand_alone_program():
    subprocess.check_call(["make", "-s", "-C", M.HOSTCHECK_DIR, "san"])
    out = subprocess.run([os.path.join(M.HOSTCHECK_DIR, "hostcheck_cloudmap_san")], capture_output=True, text=True, timeout=300)
    text = out.stdout + out.stderr
    assert out.returncode == 0 and "hostcheck_cloudmap ok" in out.stdout, text[-3000:]
    assert "runtime error" not in text and "AddressSanitizer" not in text, text[-3000:]
