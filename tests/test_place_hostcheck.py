"""CPU-only: place_math.h — the per-point classification of a scan descriptor, the quantised cosine of two columns and the distance
of a shift (loam_amd/csrc/place_kernels.hip; include/loamx.h, "place recognition") — compiled with g++ -O2 -ffp-contract=off
(tests/hostcheck_place) against the numpy model of tests/place_common.py: equality of cells, codes, cosines and of the bits of
the distances. `make san` builds the same functions into a stand-alone program under ASan + UBSan, which is run as it is.

One ring (R = 1) makes every column a single number, every cosine 1 and every shift a tie at distance 0: the shift of a rolled
descriptor is asserted at R >= 3 only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import place_common as M

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "hostcheck_place")
SHAPES = [(1, 3), (3, 5), (20, 60), (64, 360)]
L, Z_OFFSET, Z_SCALE = 80.0, 2.0, 64.0
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", DIR])
        _lib = C.CDLL(os.path.join(DIR, "libhostcheck_place.so"))
        _lib.hostcheck_place_pair.restype = C.c_uint32
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def dirs_of(S):
    d = np.zeros((S, 2))
    lib().hostcheck_place_dirs(C.c_uint32(S), _p(d))
    return d


def header_cells(pts, R, S, dirs, max_range=L, z_offset=Z_OFFSET, z_scale=Z_SCALE):
    pts = np.ascontiguousarray(np.asarray(pts, dtype=np.float64).reshape(-1, 3))
    cell, code = np.zeros(len(pts), dtype=np.uint32), np.zeros(len(pts), dtype=np.uint32)
    lib().hostcheck_place_cells(C.c_uint32(R), C.c_uint32(S), C.c_double(max_range), C.c_double(z_offset), C.c_double(z_scale), _p(dirs), _p(pts),
                                C.c_uint64(len(pts)), _p(cell), _p(code))
    return np.where(cell == 0xFFFFFFFF, -1, cell.astype(np.int64)), code.astype(np.int64)


def header_pair(q, e):
    q, e = np.ascontiguousarray(q, dtype=np.uint16), np.ascontiguousarray(e, dtype=np.uint16)
    R, S = q.shape
    dist = np.zeros(S)
    best = lib().hostcheck_place_pair(_p(q), _p(e), C.c_uint32(R), C.c_uint32(S), _p(dist))
    return dist, int(best)


def same_cells(pts, R, S, dirs, **kw):
    got_cell, got_code = header_cells(pts, R, S, dirs, **kw)
    want_cell, want_code = M.classify(pts, dirs, R, kw.get("max_range", L), kw.get("z_offset", Z_OFFSET), kw.get("z_scale", Z_SCALE))
    bad = np.flatnonzero((got_cell != want_cell) | ((want_cell >= 0) & (got_code != want_code)))
    assert not len(bad), (R, S, len(bad), bad[:5].tolist(), np.asarray(pts).reshape(-1, 3)[bad[:5]].tolist(), got_cell[bad[:5]].tolist(),
                          want_cell[bad[:5]].tolist(), got_code[bad[:5]].tolist(), want_code[bad[:5]].tolist())
    return want_cell, want_code


def test_the_sector_table_is_the_organisers_at_azimuth_zero():
    for S in (3, 60, 360):
        d = dirs_of(S)
        phi = 2.0 * np.pi * (np.arange(S) - 0.5) / S
        assert np.abs(d - np.stack([np.cos(phi), np.sin(phi)], axis=1)).max() < 1e-15


@pytest.mark.parametrize("R,S", SHAPES)
def test_random_clouds(R, S):
    rng = np.random.default_rng([91, R, S])
    dirs = dirs_of(S)
    cell, code = same_cells(M.random_cloud(rng, 20000, -100.0, 100.0), R, S, dirs)
    assert (cell >= 0).sum() > 5000 and (cell < 0).sum() > 2000 and len(np.unique(cell)) > min(R * S, 2000) // 2


@pytest.mark.parametrize("R,S", SHAPES)
def test_ring_boundaries_the_outer_range_and_the_height_clamps(R, S):
    rng = np.random.default_rng([92, R, S])
    dirs = dirs_of(S)
    pts = []
    for r in range(R + 1):  # every ring boundary (the last is the outer range), one ulp either side, in random directions
        b = L * r / R
        for rho in (b, np.nextafter(b, 0.0), np.nextafter(b, 1e9)):
            a = rng.uniform(0, 2 * np.pi, 4)
            pts += [[rho, 0.0, 1.0], [0.0, -rho, 1.0]] + [[rho * np.cos(t), rho * np.sin(t), 1.0] for t in a]
    z_lo, z_hi = -Z_OFFSET, 65534.0 / Z_SCALE - Z_OFFSET  # h == 0 and h == 65534 exactly
    for z in (z_lo, np.nextafter(z_lo, -9), np.nextafter(z_lo, 9), z_lo + 1.0 / Z_SCALE, z_lo - 1.0, -1e150, z_hi, np.nextafter(z_hi, 0), np.nextafter(z_hi, 1e9),
              z_hi + 1.0 / Z_SCALE, z_hi + 10.0, 1e150, 0.0, -0.0):
        pts += [[3.0, 4.0, z], [-7.0, 0.5, z]]
    cell, code = same_cells(pts, R, S, dirs)
    n_z = 14 * 2
    assert set(code[-n_z:][cell[-n_z:] >= 0].tolist()) >= {1, 2, 65534, 65535}
    assert cell[0] < 0 and (cell[: 6 * 3] < 0).all()  # (rho within an ulp of 0: no azimuth)
    outer = cell[-n_z - 18:-n_z].reshape(3, 6)  # at L, one ulp inside, one ulp outside
    assert (outer[0] < 0).all() and (outer[2] < 0).all() and (outer[1][:2] >= 0).all()


@pytest.mark.parametrize("R,S", SHAPES[1:])
def test_lengths_the_rho2_threshold_and_non_finite_input(R, S):
    rng = np.random.default_rng([93, R, S])
    dirs = dirs_of(S)
    pts = []
    for e in range(-49, 151, 7):  # lengths 1e-49 .. 1e150 (max_range scaled with them, so that the points stay inside)
        u = rng.standard_normal((20, 3))
        pts_e = u * 10.0 ** e
        c, k = same_cells(pts_e, R, S, dirs, max_range=10.0 ** min(e + 1, 300))
        assert (c >= 0).sum() >= 5, e
    thr = [[1e-50, 0.0, 1.0], [np.nextafter(1e-50, 0), 0.0, 1.0], [np.nextafter(1e-50, 1), 0.0, 1.0], [7e-51, 7.2e-51, 0.0], [7e-51, 7e-51, 0.0],
           [1e-51, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 5.0], [-0.0, 0.0, -0.0]]
    c, k = same_cells(thr, R, S, dirs)
    assert (c >= 0).any() and (c < 0).any()
    bad = [[np.nan, 1, 1], [1, np.nan, 1], [1, 1, np.nan], [np.inf, 1, 1], [1, -np.inf, 1], [1, 1, np.inf], [1e200, 1, 1], [1, 1, 1e200],
           [1.2e154, 1.2e154, 0.0]]
    c, k = same_cells(bad, R, S, dirs)
    assert (c < 0).all()
    same_cells(M.random_cloud(rng, 500).astype(np.float32), R, S, dirs)  # (float input is widened first)


def test_cosines_at_the_largest_values_the_clamp_and_random_sums():
    rng = np.random.default_rng(94)
    big = np.uint64(64 * 65535 ** 2)
    dot = np.concatenate([[big, big, 0, 1, 10, 3, 2 ** 40], rng.integers(0, 2 ** 38, 5000, dtype=np.uint64)]).astype(np.uint64)
    nq = np.concatenate([[big, big, 5, 1, 1, 9, 1], rng.integers(1, 2 ** 38, 5000, dtype=np.uint64)]).astype(np.uint64)
    ne = np.concatenate([[big, 1, 7, 1, 1, 1, 1], rng.integers(1, 2 ** 38, 5000, dtype=np.uint64)]).astype(np.uint64)
    # (most random triples break Cauchy-Schwarz: what matters is that header and model treat the same doubles alike)
    k = np.zeros(len(dot), dtype=np.uint64)
    lib().hostcheck_place_cos(_p(dot), _p(nq), _p(ne), C.c_uint64(len(dot)), _p(k))
    want = M.cos_q(dot, nq, ne)
    assert k[0] == M.COS_ONE and k[2] == 0 and k[3] == M.COS_ONE and k[4] == M.COS_ONE and k[5] == M.COS_ONE and k[6] == M.COS_ONE
    assert (k <= M.COS_ONE).all() and (k < M.COS_ONE).sum() > 100
    assert np.array_equal(k, want)
    # a column against itself is 1.0 exactly, whatever its norm
    n = np.concatenate([np.arange(1, 2000, dtype=np.uint64), rng.integers(1, 64 * 65535 ** 2, 5000, dtype=np.uint64), [big]]).astype(np.uint64)
    k = np.zeros(len(n), dtype=np.uint64)
    lib().hostcheck_place_cos(_p(n), _p(n), _p(n), C.c_uint64(len(n)), _p(k))
    assert (k == M.COS_ONE).all()


def test_shift_distances_from_scores_and_no_counted_column():
    score = np.array([0, 0, 1, 2 ** 30, 2 ** 30 - 1, 360 * 2 ** 30, 360 * 2 ** 30 - 1, 123456789012], dtype=np.uint64)
    m = np.array([0, 5, 1, 1, 1, 360, 360, 200], dtype=np.uint32)
    dist = np.zeros(len(m))
    lib().hostcheck_place_shift_distance(_p(score), _p(m), C.c_uint64(len(m)), _p(dist))
    want = [1.0 if mm == 0 else np.float64(1.0) - np.float64(int(s)) / (np.float64(int(mm)) * np.float64(2 ** 30)) for s, mm in zip(score, m)]
    assert dist.tobytes() == np.array(want).tobytes()
    assert dist[0] == 1.0 and dist[1] == 1.0 and dist[3] == 0.0 and dist[5] == 0.0 and dist[4] > 0.0


@pytest.mark.parametrize("R,S", SHAPES)
def test_descriptor_pairs(R, S):
    rng = np.random.default_rng([95, R, S])
    d = M.random_descriptors(rng, 3, R, S, hi=65536)
    full, none = np.full((R, S), 65535, np.uint16), np.zeros((R, S), np.uint16)
    sparse = d[2].copy()
    sparse[:, ::2] = 0
    for q, e in ((d[0], d[1]), (d[0], d[0]), (full, full), (full, d[1]), (none, d[0]), (d[0], none), (sparse, np.roll(sparse, 1, axis=1)),
                 (sparse, d[1])):
        got, best = header_pair(q, e)
        want = M.shift_distances(q, e)
        assert got.tobytes() == want.tobytes(), (R, S, got[:4], want[:4])
        assert best == int(np.argmin(want))
    got, best = header_pair(none, d[0])
    assert (got == 1.0).all() and best == 0  # m == 0 under every shift
    got, best = header_pair(full, full)
    assert (got == 0.0).all() and best == 0  # the largest dots and norms: 64 x 65535^2 at R = 64
    if R >= 3:
        d[0][0, :] = np.arange(1, S + 1)
        for s in range(0, S, 7 if S > 6 else 1):
            got, best = header_pair(np.roll(d[0], -s, axis=1), d[0])
            assert best == s and got[s] == 0.0, (R, S, s, best)


def test_the_model_itself_on_a_case_worked_by_hand():
    """S = 3, R = 2, max_range 2: one point per sector at azimuths 0, 120 and 240 degrees, rings 0, 1, 1"""
    dirs = dirs_of(3)
    pts = np.array([[0.5, 0.0, 0.0], [1.5 * np.cos(2.0), 1.5 * np.sin(2.0), -1.0], [1.5 * np.cos(4.2), 1.5 * np.sin(4.2), 1.0], [2.5, 0.0, 9.0]])
    d = M.descriptor(pts, dirs, n_rings=2, max_range=2.0, z_offset=2.0, z_scale=64.0)
    assert d.tolist() == [[129, 0, 0], [0, 65, 193]]
    assert M.ring_keys(d).tolist() == [129, 258] and M.column_norms(d).tolist() == [129 ** 2, 65 ** 2, 193 ** 2]
    q = np.roll(d, -1, axis=1)
    assert M.pair_distance(q, d) == (0.0, 1)
    rec = M.search(q, np.stack([d, q]), 3, None)
    assert rec["id"].tolist() == [0, 1, M.NO_ID] and rec["shift"].tolist() == [1, 0, 0] and rec["distance"].tolist() == [0.0, 0.0, 2.0]


def test_the_sanitizer_build_runs_clean():
    subprocess.check_call(["make", "-s", "-C", DIR, "san"])
    out = subprocess.run([os.path.join(DIR, "hostcheck_place_san")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "hostcheck_place ok" in out.stdout
