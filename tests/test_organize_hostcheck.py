"""CPU-only: organize_math.h — the two tables of a scan layout and the per-point classification of the organise kernels
(loam_amd/csrc/organize_kernels.hip; include/loamx.h, "unordered clouds into scans") — compiled with g++ -O2 -ffp-contract=off
(tests/hostcheck_organize) against the numpy model of tests/organize_common.py (equality of cells and of the bits of r2) and,
for the tables, against 40-digit mpmath arithmetic.

The measure of the tables: for a column boundary |u_k - (cos phi_k, sin phi_k)| with phi_k formed at 40 digits from the DOUBLE
azimuth_zero; for a line boundary |t_l - tan(b_l)| / (1 + tan(b_l)^2) with b_l formed at 40 digits from the DOUBLE elevations,
i.e. the error as an angle. Measured with g++ -O2 -ffp-contract=off and glibc on x86-64 over every layout below: worst column
error 1.5e-15 (MEASURED_COL: W = 256, azimuth_zero = 6: the double phi_k lies near 12 there and its own rounding, half an ulp, is
8.9e-16; with azimuth_zero = 0 the worst is 8.0e-16), worst line error 1.3e-16 (MEASURED_LINE). Asserted: 8 x that, libm's sin / cos / tan differing between
machines by an ulp or so.

Where the rule has no answer, and what the header does there (none of it is reached by the model, which asserts uniqueness):
W == 1 has one boundary and no c with s_c true and s_(c + 1) false; the column is 0. At W == 2 the two boundaries are half a
turn apart, so a point within rounding of either makes both signs agree; the header then answers 1 (= W / 2). The boundary cases
below therefore run at W >= 3 (W = 37, 1024, 4096)."""
import ctypes as C
import os
import subprocess

import mpmath
import numpy as np
import pytest

import organize_common as M

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "hostcheck_organize")
MEASURED_COL = 1.5e-15
MEASURED_LINE = 1.3e-16
FACTOR = 8
SHAPES = [(1, 1), (2, 2), (8, 37), (64, 1024), (128, 4096)]
_lib = None
mp = mpmath.mp.clone()
mp.dps = 40


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", DIR])
        _lib = C.CDLL(os.path.join(DIR, "libhostcheck_organize.so"))
    return _lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def tables(H, W, azimuth_zero=0.0, clockwise=False, elevations=None, fov=(-0.4, 0.2)):
    """(col_dirs (W, 2), line_tans (H + 1,)) or None when the header refuses the elevations"""
    col, tan = np.zeros((W, 2)), np.zeros(H + 1)
    el = None if elevations is None else np.ascontiguousarray(elevations, dtype=np.float64)
    rc = lib().hostcheck_organize_tables(C.c_double(azimuth_zero), C.c_int(1 if clockwise else 0), _dp(el) if el is not None else None,
                                         C.c_double(fov[0]), C.c_double(fov[1]), C.c_uint32(H), C.c_uint32(W), _dp(col), _dp(tan))
    return None if rc else (col, tan)


def header_cells(pts, col, tan, clockwise=False, rings=None, ring_map=None):
    pts = np.ascontiguousarray(np.asarray(pts, dtype=np.float64).reshape(-1, 3))
    n, W, H = len(pts), len(col), len(tan) - 1
    cell, r2 = np.zeros(n, dtype=np.uint32), np.zeros(n)
    u16p = C.POINTER(C.c_uint16)
    rg = None if rings is None else np.ascontiguousarray(rings, dtype=np.uint16)
    rm = None if ring_map is None else np.ascontiguousarray(ring_map, dtype=np.uint16)
    lib().hostcheck_organize_cells(_dp(np.ascontiguousarray(col)), _dp(np.ascontiguousarray(tan)), C.c_uint32(H), C.c_uint32(W),
                                   C.c_int(1 if clockwise else 0), rm.ctypes.data_as(u16p) if rm is not None else None,
                                   C.c_uint32(0 if rm is None else len(rm)), _dp(pts), rg.ctypes.data_as(u16p) if rg is not None else None,
                                   C.c_uint64(n), cell.ctypes.data_as(C.POINTER(C.c_uint32)), _dp(r2))
    return cell, r2


def agree(what, pts, col, tan, clockwise=False, rings=None, ring_map=None):
    """header == model: the cells, and the bits of r2 for every point that is not invalid; returns the cells"""
    got, r2 = header_cells(pts, col, tan, clockwise, rings, ring_map)
    want, r2_want = M.classify(np.asarray(pts, dtype=np.float64).reshape(-1, 3), col, tan, clockwise, rings, ring_map)
    bad = np.flatnonzero(got != want)
    assert not len(bad), (what, len(bad), bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())
    live = got != M.INVALID
    assert np.array_equal(r2[live].view(np.uint64), r2_want[live].view(np.uint64)), what
    return got


@pytest.mark.parametrize("H,W", SHAPES)
def test_twenty_thousand_random_points_land_where_the_model_puts_them(H, W):
    rng = np.random.default_rng([41, H, W])
    col, tan = tables(H, W)
    pts = M.random_cloud(rng, 20000)
    pts[:5000] *= np.exp(rng.uniform(np.log(1e-3), np.log(1e3), 5000))[:, None]
    cell = agree("random %d x %d" % (H, W), pts, col, tan)
    placed = cell < M.INVALID
    assert placed.sum() > 5000 and (cell == M.OUTSIDE).sum() > (100 if H > 1 else -1)
    if H > 1:
        assert len(np.unique(cell[placed] // W)) == H
    assert len(np.unique(cell[placed] % W)) >= min(W, 1000)
    # the default convention: column c is centred on the azimuth 2 pi c / W
    az = np.arctan2(pts[placed, 1], pts[placed, 0])
    d = np.angle(np.exp(1j * (az - 2 * np.pi * (cell[placed] % W) / W)))
    assert np.abs(d).max() <= np.pi / W * (1 + 1e-9)


@pytest.mark.parametrize("H,W", [(8, 37), (64, 1024), (128, 4096)])
@pytest.mark.parametrize("clockwise,az0", [(False, 0.0), (True, 0.3)])
def test_a_point_on_a_column_boundary_belongs_to_the_column_that_starts_there(H, W, clockwise, az0):
    """rho u_k with rho a power of two: both products of the cross product are the same double, the difference is exactly 0
    and s_k is true. A step along the tangent, taken in the coordinate the tangent is steepest in (|u| >= 0.707 there), falls to
    either side: ahead of the boundary one ulp stays in column k; behind it one ulp falls into column k - 1 UNLESS the product
    u x absorbs it — a product of a factor in [0.707, 1] moves by 0.7 to 1 ulp of itself when the other factor moves by one ulp,
    and two reals less than an ulp apart can round to the same double — in which case the cross product is still exactly 0
    and the point still belongs to k (measured: 23 of 1 024 and 128 of 4 096 boundaries). Two ulps move the product by at least 1.41 of its
    ulps, which no rounding absorbs: they always fall into k - 1."""
    col, tan = tables(H, W, az0, clockwise)
    k = np.arange(W)
    sgn = -1.0 if clockwise else 1.0
    along_y = np.abs(col[:, 0]) >= np.abs(col[:, 1])
    for rho in (0.125, 1.0, 32.0):
        p = np.stack([rho * col[:, 0], rho * col[:, 1], np.zeros(W)], axis=1)
        cell = agree("on boundary", p, col, tan, clockwise)
        assert (cell < M.INVALID).all() and np.array_equal(cell % W, k), (rho, np.flatnonzero(cell % W != k)[:5])
        for side in (+1.0, -1.0):
            # the tangent in the sense of counting is sgn (-u.y, u.x)
            ty, tx = side * sgn * col[:, 0], -side * sgn * col[:, 1]
            q = p.copy()
            for ulps in (1, 2):
                q[along_y, 1] = np.nextafter(q[along_y, 1], np.where(ty[along_y] > 0, np.inf, -np.inf))
                q[~along_y, 0] = np.nextafter(q[~along_y, 0], np.where(tx[~along_y] > 0, np.inf, -np.inf))
                got = agree("beside boundary", q, col, tan, clockwise)
                assert np.array_equal(got // W, cell // W)
                if side > 0:
                    assert np.array_equal(got % W, k), (rho, ulps, np.flatnonzero(got % W != k)[:5])
                    continue
                cross = col[:, 0] * q[:, 1] - col[:, 1] * q[:, 0]
                want = np.where(cross == 0.0, k, (k - 1) % W)
                assert np.array_equal(got % W, want), (rho, ulps, np.flatnonzero(got % W != want)[:5])
                print("W", W, "rho", rho, ulps, "ulp behind the boundary:", int((cross == 0.0).sum()), "of", W, "still on it")
                if ulps == 1:
                    assert (cross != 0.0).mean() > 0.5
                else:
                    assert (cross != 0.0).all()


@pytest.mark.parametrize("H,W", [(2, 2), (8, 37), (64, 1024)])
def test_a_point_on_a_line_boundary_belongs_to_the_line_above_it(H, W):
    """(rho, 0, t_l rho) with rho a power of two: rho2 and its root are exact and so is the product, z >= t_l rho holds"""
    el = np.sort(np.random.default_rng(5).uniform(-0.45, 0.3, H)) if H > 2 else None
    col, tan = tables(H, W, elevations=el)
    l = np.arange(H + 1)
    for rho in (0.25, 1.0, 64.0):
        p = np.stack([np.full(H + 1, rho), np.zeros(H + 1), tan * rho], axis=1)
        cell = agree("on line boundary", p, col, tan)
        assert np.array_equal(cell[:H], l[:H] * W) and cell[H] == M.OUTSIDE
        below = p.copy()
        below[:, 2] = np.nextafter(p[:, 2], -np.inf)
        cell = agree("below line boundary", below, col, tan)
        assert cell[0] == M.OUTSIDE and np.array_equal(cell[1:], l[:H] * W)


@pytest.mark.parametrize("H,W", [(8, 37), (64, 1024)])
def test_lengths_from_1e_minus_49_to_1e150_and_the_threshold_of_rho2(H, W):
    rng = np.random.default_rng([43, H, W])
    col, tan = tables(H, W)
    d = M.random_cloud(rng, 4000, -1.0, 1.0)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    scale = np.exp(rng.uniform(np.log(1e-49), np.log(1e150), 4000))
    scale[:4] = [1e-49, 1e150, 1e-30, 1e100]
    cell = agree("scaled", d * scale[:, None], col, tan)
    same = agree("unit", d, col, tan)
    far = np.abs(d[:, :2]).max(axis=1) > 0.1  # (away from the pole the cell of a direction does not depend on the length:
    assert (cell[far] == same[far]).mean() > 0.999  # up to the roundings at a boundary)
    assert (cell < M.INVALID).sum() > 1000
    # rho2 at and just below 1e-100; r2 beyond the doubles
    x = 1e-50
    while x * x >= 1e-100:
        x = np.nextafter(x, 0.0)
    while x * x < 1e-100:
        x = np.nextafter(x, 1.0)
    lo = np.nextafter(x, 0.0)
    pts = np.array([[x, 0.0, 0.0], [lo, 0.0, 0.0], [0.0, -x, 1.0], [0.0, lo, 1.0], [-x, 0.0, -5e-51], [1e154, 1e154, 0.0], [1.0, 1.0, 1e155],
                    [1e153, 1.0, 1e153]])
    cell = agree("threshold", pts, col, tan)
    assert [int(c == M.INVALID) for c in cell] == [0, 1, 0, 1, 0, 1, 1, 0]


def test_non_finite_coordinates_and_points_on_the_axis_are_invalid():
    col, tan = tables(8, 37)
    pts = []
    for bad in (np.nan, np.inf, -np.inf):
        for i in range(3):
            p = [1.5, -2.0, 0.25]
            p[i] = bad
            pts.append(p)
    pts += [[0.0, 0.0, 0.0], [-0.0, 0.0, -0.0], [0.0, 0.0, 3.0], [0.0, -0.0, -1e300], [1e-60, 1e-60, 1.0], [np.nan, np.nan, np.nan]]
    cell = agree("invalid", pts, col, tan)
    assert (cell == M.INVALID).all()
    rings = np.zeros(len(pts), dtype=np.uint16)
    assert (agree("invalid with rings", pts, col, tan, rings=rings) == M.INVALID).all()


@pytest.mark.parametrize("H,W", [(8, 37), (16, 128)])
def test_clockwise_with_an_azimuth_zero_uneven_elevations_and_rings(H, W):
    rng = np.random.default_rng([47, H, W])
    el = np.sort(rng.uniform(-0.5, 0.35, H))
    col, tan = tables(H, W, 0.3, True, el)
    pts = M.random_cloud(rng, 6000)
    cell = agree("clockwise", pts, col, tan, True)
    placed = cell < M.INVALID
    az = np.arctan2(pts[placed, 1], pts[placed, 0])
    d = np.angle(np.exp(1j * (az - (0.3 - 2 * np.pi * (cell[placed] % W) / W))))
    assert np.abs(d).max() <= np.pi / W * (1 + 1e-9)
    elev = np.arctan2(pts[placed, 2], np.hypot(pts[placed, 0], pts[placed, 1]))
    assert (np.abs(elev - el[cell[placed] // W]) <= np.abs(elev[:, None] - el[None, :]).min(axis=1) + 1e-12).all()  # the nearest beam
    # rings: as they are, through a permuting map with a dropped ring, beyond the map, beyond the lines
    rings = rng.integers(0, H + 3, len(pts)).astype(np.uint16)
    got = agree("rings", pts, col, tan, True, rings=rings)
    assert ((got == M.OUTSIDE) == (rings >= H)).all()
    ring_map = np.append(rng.permutation(H), [0xFFFF]).astype(np.uint16)
    got = agree("ring map", pts, col, tan, True, rings=rings, ring_map=ring_map)
    assert ((got == M.OUTSIDE) == (rings >= H)).all()
    inside = rings < H
    assert np.array_equal(got[inside] // W, ring_map[rings[inside]])


def test_the_elevations_the_layout_refuses():
    assert tables(4, 8, elevations=[-0.2, -0.1, 0.0, 0.1]) is not None
    assert tables(4, 8, elevations=[-0.2, -0.1, -0.1, 0.1]) is None      # not strictly ascending
    assert tables(4, 8, elevations=[0.1, 0.0, -0.1, -0.2]) is None
    assert tables(4, 8, elevations=[-0.2, np.nan, 0.0, 0.1]) is None
    assert tables(4, 8, elevations=[-0.2, -0.1, 0.0, np.inf]) is None
    assert tables(2, 8, elevations=[-1.5, -1.3]) is None                   # the lower boundary at -1.6 < -pi / 2
    assert tables(2, 8, elevations=[1.0, 1.4]) is None                     # the upper boundary at 1.6
    assert tables(2, 8, elevations=[1.0, 1.3]) is not None
    assert tables(4, 8, fov=(0.2, 0.2)) is None and tables(4, 8, fov=(0.2, -0.2)) is None
    assert tables(1, 8, fov=(0.2, -0.2)) is not None                       # one line: no fan to speak of
    col, tan = tables(1, 8, elevations=[0.1])
    assert tan.tolist() == [-np.inf, np.inf]


def table_errors(H, W, az0, clockwise, el, fov):
    col, tan = tables(H, W, az0, clockwise, el, fov)
    sgn = -1 if clockwise else 1
    worst_col = 0.0
    for k in range(W):
        phi = mp.mpf(float(az0)) + sgn * 2 * mp.pi * (mp.mpf(k) - mp.mpf(1) / 2) / W
        worst_col = max(worst_col, float(mp.sqrt((mp.mpf(float(col[k, 0])) - mp.cos(phi)) ** 2 + (mp.mpf(float(col[k, 1])) - mp.sin(phi)) ** 2)))
    worst_line = 0.0
    if H > 1:
        if el is None:
            # (the linear fan's elevations are doubles the header forms; the boundaries are measured from them)
            e = [mp.mpf(float(fov[0] + (fov[1] - fov[0]) * float(i) / float(H - 1))) for i in range(H)]
        else:
            e = [mp.mpf(float(v)) for v in el]
        b = [e[0] - (e[1] - e[0]) / 2] + [(e[i - 1] + e[i]) / 2 for i in range(1, H)] + [e[-1] + (e[-1] - e[-2]) / 2]
        for i in range(H + 1):
            t = mp.tan(b[i])
            worst_line = max(worst_line, float(abs(mp.mpf(float(tan[i])) - t) / (1 + t * t)))
    return worst_col, worst_line


def test_the_tables_against_mpmath_at_40_digits():
    rng = np.random.default_rng(49)
    worst_col = worst_line = 0.0
    for H, W, az0, cw, el, fov in [(1, 1, 0.0, False, None, (-0.4, 0.2)), (2, 2, 0.0, False, None, (-0.4, 0.2)),
                                   (8, 37, 0.0, False, None, (-0.4, 0.2)), (64, 1024, 0.0, False, None, (np.radians(-24.8), np.radians(2.0))),
                                   (128, 4096, 0.3, True, None, (-0.26, 0.26)), (16, 128, -2.5, True, np.sort(rng.uniform(-0.5, 0.35, 16)), None),
                                   (32, 256, 6.0, False, np.sort(rng.uniform(-1.4, 1.4, 32)), None)]:
        c, l = table_errors(H, W, az0, cw, el, fov or (0.0, 0.0))
        print("tables %d x %d az0 %g cw %d: column error %.3g, line error %.3g" % (H, W, az0, cw, c, l))
        worst_col, worst_line = max(worst_col, c), max(worst_line, l)
    print("worst column error", worst_col, "limit", FACTOR * MEASURED_COL, "; worst line error", worst_line, "limit", FACTOR * MEASURED_LINE)
    assert 0.0 < worst_col <= FACTOR * MEASURED_COL
    assert 0.0 < worst_line <= FACTOR * MEASURED_LINE


def test_the_same_functions_are_clean_under_asan_and_ubsan_in_a_stand_alone_program():
    subprocess.check_call(["make", "-s", "-C", DIR, "san"])
    out = subprocess.run([os.path.join(DIR, "hostcheck_organize_san")], capture_output=True, text=True, timeout=300)
    text = out.stdout + out.stderr
    assert out.returncode == 0 and "hostcheck_organize ok" in out.stdout, text[-3000:]
    assert "runtime error" not in text and "AddressSanitizer" not in text, text[-3000:]
