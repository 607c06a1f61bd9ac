"""CPU-only: segment_math.h — the validity, ground-pair and edge predicates of the segmentation kernels
(loam_amd/csrc/segment_kernels.hip) — compiled with g++ (tests/hostcheck_segment) against the numpy model of
tests/segment_common.py, bit for bit, and a serial union-find over the same predicates against the model's components. The GPU
tests (test_gpu_segment.py) compare the kernels with the same model."""
import ctypes as C
import os
import subprocess

import numpy as np

import segment_common as M
from loam_amd import capi

HOSTCHECK_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck_segment")
dp, u8p, u32p = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", HOSTCHECK_DIR])
        _lib = C.CDLL(os.path.join(HOSTCHECK_DIR, "libhostcheck_segment.so"))
    return _lib


def _p(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3)


def header_valid(p, lo, hi):
    p = _p(p)
    out = np.zeros(len(p), np.uint8)
    lib().hostcheck_segment_valid(p.ctypes.data_as(dp), C.c_uint64(len(p)), C.c_double(lo), C.c_double(hi), out.ctypes.data_as(u8p))
    return out.astype(bool)


def header_pairs(fn, a, b, k):
    a, b = _p(a), _p(b)
    out = np.zeros(len(a), np.uint8)
    getattr(lib(), fn)(a.ctypes.data_as(dp), b.ctypes.data_as(dp), C.c_uint64(len(a)), C.c_double(k), out.ctypes.data_as(u8p))
    return out.astype(bool)


def fuzz_points(rng, n):
    """directions times magnitudes from 1e-30 to 1e30, a third of them float32 values widened"""
    p = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-30, 30, (n, 1))
    p[::3] = p[::3].astype(np.float32).astype(np.float64)
    p[1::7] = rng.normal(size=(len(p[1::7]), 3)) * 30.0  # (ordinary ranges)
    return p


def on_the_threshold(pred, make_b, lo, hi):
    """Per pair: bisects the scale s in [lo, hi] (pred true at lo, false at hi) until two neighbouring doubles straddle the
    threshold, then returns b at both of them and one ulp further each way."""
    assert pred(make_b(lo)).all() and not pred(make_b(hi)).any()
    for _ in range(80):
        mid = lo + (hi - lo) / 2
        t = pred(make_b(mid))
        lo, hi = np.where(t, mid, lo), np.where(t, hi, mid)
    assert (np.nextafter(lo, np.inf) == hi).all()
    return [make_b(s) for s in (np.nextafter(lo, -np.inf), lo, hi, np.nextafter(hi, np.inf))]


def test_validity_bit_for_bit():
    rng = np.random.default_rng(31)
    for lo, hi in ((1.0, 120.0), (0.0, 1e30), (2.0, 2.0), (0.5, 1e-3)):
        r = np.array([lo, np.nextafter(lo, 0), np.nextafter(lo, np.inf), hi, np.nextafter(hi, 0), np.nextafter(hi, np.inf), 0.0, 1e200, 1e-200])
        special = [[np.nan, 0, 0], [0, -np.inf, 0], [0, 5, np.inf], [1e155, 1e155, 0], [0, 0, 0], [-0.0, -0.0, -0.0], [1e200, 0, 0]]
        pts = np.concatenate([np.stack([r, 0 * r, 0 * r], 1), np.stack([0 * r, -r, 0 * r], 1), fuzz_points(rng, 20000), rng.normal(size=(5000, 3)) * 60, special])
        got, want = header_valid(pts, lo, hi), M.valid_cells(pts, lo, hi)
        assert np.array_equal(got, want), (lo, hi, np.flatnonzero(got != want)[:5])
    assert header_valid([[0, 0, 0], [1, 0, 0], [np.nextafter(1, 0), 0, 0], [120, 0, 0], [np.nextafter(120, 200), 0, 0], [np.nan, 1, 1], [1e200, 0, 0]],
                        1.0, 120.0).tolist() == [False, True, False, True, False, False, False]


def test_ground_pair_bit_for_bit_on_and_next_to_the_threshold():
    rng = np.random.default_rng(32)
    tg2s = [capi.segment_constants(capi.SegmentParams(ground_angle=a))[0] for a in (np.radians(10.0), 1e-9, 0.0, 1.5)] + [1.0]
    for tg2 in tg2s:
        a, b = fuzz_points(rng, 20000), fuzz_points(rng, 20000)
        assert np.array_equal(header_pairs("hostcheck_segment_ground_pair", a, b, tg2), M.ground_pair(a, b, tg2)), tg2
        # near pairs: b a step away from a at slopes around the threshold
        a = rng.normal(size=(20000, 3)) * 30
        d = rng.normal(size=(20000, 3))
        d[:, 2] = np.sqrt(tg2 * (d[:, 0] ** 2 + d[:, 1] ** 2)) * rng.choice([1.0, 1.0 + 1e-15, 1.0 - 1e-15, 0.5, 2.0], 20000)
        assert np.array_equal(header_pairs("hostcheck_segment_ground_pair", a, a + d, tg2), M.ground_pair(a, a + d, tg2)), tg2
    # constructed: the height of b scaled until both sides meet, then one ulp each way
    tg2 = tg2s[0]
    n = 4000
    a = rng.normal(size=(n, 3)) * 20
    step = rng.uniform(0.2, 3.0, (n, 2))
    make_b = lambda s: np.stack([a[:, 0] + step[:, 0], a[:, 1] + step[:, 1], a[:, 2] + s], 1)
    for k, b in enumerate(on_the_threshold(lambda b: M.ground_pair(a, b, tg2), make_b, np.zeros(n), np.full(n, 10.0))):
        got = header_pairs("hostcheck_segment_ground_pair", a, b, tg2)
        assert np.array_equal(got, M.ground_pair(a, b, tg2))
        assert k != 1 or got.all(), "the last height on the ground side"
        assert k != 2 or not got.any(), "the first height beyond it"
    exact = header_pairs("hostcheck_segment_ground_pair", [[1, 1, 1]] * 2, [[4, 5, 6], [4, 5, np.nextafter(6, 7)]], 1.0)
    assert exact.tolist() == [True, False]  # 25 <= 25: equality is ground


def test_edge_predicate_bit_for_bit_on_and_next_to_the_threshold():
    rng = np.random.default_rng(33)
    c2s = [capi.segment_constants(capi.SegmentParams(segment_angle=a))[1] for a in (np.radians(60.0), np.radians(10.0), 1.5, 1e-6)] + [1.0]
    for c2 in c2s:
        a, b = fuzz_points(rng, 20000), fuzz_points(rng, 20000)
        got = header_pairs("hostcheck_segment_connected", a, b, c2)
        assert np.array_equal(got, M.connected(a, b, c2)), c2
        assert np.array_equal(got, header_pairs("hostcheck_segment_connected", b, a, c2)), "not symmetric"
        # neighbouring beams: a small angle apart, range ratios around the threshold
        a = rng.normal(size=(20000, 3)) * 30
        b = (a + np.cross(a, rng.normal(size=(20000, 3))) * 0.01) * rng.uniform(0.5, 2.0, (20000, 1))
        got = header_pairs("hostcheck_segment_connected", a, b, c2)
        assert np.array_equal(got, M.connected(a, b, c2)), c2
        assert np.array_equal(got, header_pairs("hostcheck_segment_connected", b, a, c2)), "not symmetric"
    c2 = c2s[0]
    n = 4000
    a = rng.normal(size=(n, 3)) * 20
    b0 = a + np.cross(a, rng.normal(size=(n, 3))) * 0.01  # (about half a degree away, nearly the same range: connected)
    make_b = lambda s: b0 * s[:, None]
    for k, b in enumerate(on_the_threshold(lambda b: M.connected(a, b, c2), make_b, np.ones(n), np.full(n, 50.0))):
        got = header_pairs("hostcheck_segment_connected", a, b, c2)
        assert np.array_equal(got, M.connected(a, b, c2))
        assert np.array_equal(got, header_pairs("hostcheck_segment_connected", b, a, c2))
        assert k != 1 or got.all(), "the last scale on the connected side"
        assert k != 2 or not got.any(), "the first scale beyond it"
    exact = header_pairs("hostcheck_segment_connected", [[1, 0, 0]] * 2, [[2, 0, 0], [2, 0.5, 0]], 1.0)
    assert exact.tolist() == [False, True]  # 4 < 4 is false: equality is not connected; 5.0625 < 5.3125 is


def serial(scan, H, W, params=None, min_range=1.0, max_range=120.0):
    params = params or capi.SegmentParams()
    tg2, c2 = capi.segment_constants(params)
    p = _p(scan)
    n = H * W
    classes, labels, sizes, spans = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    lib().hostcheck_segment_scan(p.ctypes.data_as(dp), C.c_uint32(H), C.c_uint32(W), C.c_uint32(int(params.ground_lines)), C.c_double(min_range),
                                 C.c_double(max_range), C.c_double(tg2), C.c_double(c2), C.c_uint32(int(params.min_cluster_points)),
                                 C.c_uint32(int(params.min_tall_cluster_points)), C.c_uint32(int(params.min_tall_cluster_lines)),
                                 classes.ctypes.data_as(u8p), labels.ctypes.data_as(u32p), sizes.ctypes.data_as(u32p), spans.ctypes.data_as(u32p))
    return classes, labels, sizes, spans


def same_as_model(scan, H, W, params=None, where=""):
    classes, labels, sizes, spans = serial(scan, H, W, params)
    m = M.segment(scan, H, W, params=params)
    assert np.array_equal(classes, m.classes) and np.array_equal(labels, m.labels) and np.array_equal(sizes, m.sizes), where
    span_of = {int(c["root"]): int(c["line_max"]) - int(c["line_min"]) + 1 for c in m.clusters}
    for root, span in span_of.items():
        assert spans[root] == span and (spans[labels == root] == span).all(), (where, root)
    assert (spans[labels == M.NO_LABEL] == 0).all()
    return m


def test_serial_union_find_over_the_header_gives_the_models_components():
    mp = capi.SegmentParams(**M.MASK_PARAMS)
    for H, W in ((8, 37), (19, 300), (5, 16), (1, 16), (2, 2), (3, 1)):
        for seed, far in ((1, 20.0), (2, None)):
            same_as_model(M.mask_scan(M.random_mask(H, W, seed), far=far), H, W, mp, ("random", H, W, far))
        for make in (M.serpentine, M.comb, M.alternating_lines, M.checkerboard):
            same_as_model(M.mask_scan(make(H, W)), H, W, mp, (make.__name__, H, W))
        same_as_model(M.floor_scan(H, W), H, W, where=("floor", H, W))
    for name in ("canyon", "lot", "field"):
        for params in (None, capi.SegmentParams(ground_lines=12, min_cluster_points=10), capi.SegmentParams(segment_angle=np.radians(30.0))):
            same_as_model(M.real_scan(name), 32, 512, params, name)
        same_as_model(M.real_scan(name, dtype=np.float32), 32, 512, where=name + " f32")


def test_the_same_functions_are_clean_under_asan_and_ubsan_in_a_stand_alone_program():
    subprocess.check_call(["make", "-s", "-C", HOSTCHECK_DIR, "san"])
    out = subprocess.run([os.path.join(HOSTCHECK_DIR, "hostcheck_segment_san")], capture_output=True, text=True, timeout=300)
    text = out.stdout + out.stderr
    assert out.returncode == 0 and "hostcheck_segment ok" in out.stdout, text[-3000:]
    assert "runtime error" not in text and "AddressSanitizer" not in text, text[-3000:]
