"""CPU-only: visibility_math.h — sensor frame, cell, range band, window verdict and decision of the map cleaning kernels
(loam_amd/csrc/visibility_kernels.hip) — compiled with g++ (tests/hostcheck_visibility) against the numpy model of
tests/visibility_common.py, by equality. The GPU tests (test_gpu_visibility.py) compare the kernels with the same model."""
import os
import subprocess

import numpy as np
import pytest

import visibility_common as V
from map_common import small_pose

FAN = (15.0, -15.0)
IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


def both(points, scan, pose, H, W, tables, params=None, clockwise=False):
    got = V.header_verdicts(points, scan, pose, H, W, *tables, clockwise, params)
    want = V.verdicts(points, scan, pose, H, W, *tables, clockwise, params)
    assert np.array_equal(got[1], want[1]), "place"
    assert np.array_equal(got[0], want[0]), "verdict"
    return want


@pytest.mark.parametrize("H,W", [(16, 256), (5, 37), (2, 4), (3, 1), (3, 2)])
def test_the_header_equals_the_model_on_every_window_pose_and_scalar_type(H, W):
    rng = np.random.default_rng([31, H, W])
    tables = V.analytic_tables(H, W, FAN)
    tilted = small_pose(rng, angle=0.4, shift=3.0)
    stretched = tilted.copy()
    stretched[:4] *= 1.3  # a quaternion that is not a unit quaternion is used as given
    seen = np.zeros(5, dtype=np.int64)
    for pose in (IDENTITY, tilted, stretched):
        pts = V.CM.pose_act(pose, V.cloud(rng, 1500))
        pts = np.concatenate([pts, [[np.nan, 0, 0], [0, np.inf, 0], [1e200, 1e200, 0], pose[4:], pose[4:] + [0, 0, 5.0]]])
        for dtype in (np.float64, np.float32):
            scan = V.shell_scan(rng, H, W, dtype=dtype)
            for wl, wc in ((0, 0), (1, 1), (3, 3), (0, 3), (2, 0)):
                v, place = both(pts, scan, pose, H, W, tables, V.Params(window_lines=wl, window_cols=wc))
                seen += np.bincount(v, minlength=5)
                assert (place[-5:-1] == 0).all() and (v[-5:-1] == V.NONE).all()  # non-finite points and the sensor's own position
                assert place[-1] == 0 or pose is not IDENTITY  # straight above the sensor: no azimuth
    assert (seen > 0).all(), seen


def test_points_out_of_range_at_both_edges_and_outside_the_fan_have_no_verdict():
    H, W = 8, 64
    tables = V.analytic_tables(H, W, FAN)
    scan = V.shell_scan(np.random.default_rng(32), H, W, holes=False)
    p = V.Params(min_range=2.0, max_range=30.0)
    r = np.array([2.0, np.nextafter(2.0, 0), np.nextafter(2.0, 3), 30.0, np.nextafter(30.0, 0), np.nextafter(30.0, 31)])
    pts = np.stack([r, 0 * r, 0 * r], 1)  # (r r is exact next to 2 and 30 only in the sense that both sides compute the same product)
    v, place = both(pts, scan, IDENTITY, H, W, tables, p)
    r2 = r * r
    assert np.array_equal(place >= 1, (r2 >= 4.0) & (r2 <= 900.0)) and (place >= 1).sum() >= 2 and (place == 0).sum() >= 2
    # above and below the fan: in range, no cell, no vote; the edges of the fan from both sides
    top, bottom = V.analytic_tables(H, W, FAN)[1][[-1, 0]]
    for t, inside in ((np.nextafter(top, -np.inf), True), (top, False), (bottom, True), (np.nextafter(bottom, -np.inf), False), (2.0, False), (-2.0, False)):
        pts = np.array([[8.0, 0.0, 8.0 * t]])  # (rho = 8: the products with the tangents are exact)
        v, place = both(pts, scan, IDENTITY, H, W, tables, p)
        assert place[0] == (2 if inside else 1) and (v[0] != V.NONE) == inside, (t, place, v)


def _edge_range(bound2, first_at_least):
    """the double r nearest the bound with r r >= bound2 (first_at_least) or r r <= bound2, by bisection on the doubles"""
    lo, hi = 0.0, 1e6
    for _ in range(200):
        mid = lo + (hi - lo) / 2
        if mid == lo or mid == hi:
            break
        if mid * mid >= bound2 if first_at_least else mid * mid > bound2:
            hi = mid
        else:
            lo = mid
    return hi if first_at_least else lo


@pytest.mark.parametrize("dist,margin,rel", [(12.5, 0.3, 0.01), (3.7, 0.0, 0.0), (2.0, 5.0, 0.0), (40.0, 0.1, 0.05)])
def test_a_cell_bisected_onto_lo2_and_hi2_and_one_ulp_each_way(dist, margin, rel):
    H, W = 4, 8
    tables = V.analytic_tables(H, W, FAN)
    p = V.Params(min_range=0.0, margin=margin, margin_rel=rel, window_lines=0, window_cols=0)
    pt = np.array([[dist, 0.0, 0.0]])
    q = V.to_sensor(pt, IDENTITY)
    r2 = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
    lo2, hi2 = (float(x[0]) for x in V.bounds(r2, p))
    cell = int(V.O.classify(q, *tables)[0][0])
    if margin > dist:
        assert lo2 == 0.0  # lo was negative and is taken as 0
    r_lo, r_hi = _edge_range(lo2, True), _edge_range(hi2, False)
    cases = [(r_hi, V.AGREE), (np.nextafter(r_hi, np.inf), V.THROUGH), ((r_lo + r_hi) / 2, V.AGREE), (r_lo, V.AGREE)]
    if lo2 > 0.0:
        cases.append((np.nextafter(r_lo, 0.0), V.OCCLUDED))
    else:
        cases.append((5e-324, V.AGREE))  # with lo at 0 and no min_range every return in front of the point agrees
    for r, want in cases:
        scan = np.zeros((H * W, 3))
        scan[cell] = [r, 0.0, 0.0]  # (r2c = r r to the bit, whatever direction the cell stands for)
        v, place = both(pt, scan, IDENTITY, H, W, tables, p)
        assert place[0] == 2 and v[0] == want, (r, v, want, lo2, hi2)


def test_windows_clip_at_the_first_and_last_line_wrap_at_the_seam_and_may_lap_themselves():
    rng = np.random.default_rng(33)
    for H, W in ((4, 8), (3, 4), (3, 2), (3, 1)):
        tables = V.analytic_tables(H, W, FAN)
        el = V.O.fan_elevations(H, FAN)
        # one point per cell, at 10 m along the cell's own direction
        az = 2.0 * np.pi * np.arange(W) / W
        d = np.stack([np.cos(el)[:, None] * np.cos(az)[None, :], np.cos(el)[:, None] * np.sin(az)[None, :], np.broadcast_to(np.sin(el)[:, None], (H, W))], -1)
        pts = (10.0 * d).reshape(-1, 3)
        assert np.array_equal(V.O.classify(pts, *tables)[0], np.arange(H * W))
        for wl, wc in ((0, 0), (1, 1), (3, 3), (0, 3), (1, 0)):
            p = V.Params(window_lines=wl, window_cols=wc)
            for hot in range(H * W):  # a single agreeing return in an otherwise empty scan: AGREE exactly where the window reaches it
                scan = np.zeros((H * W, 3))
                scan[hot] = 10.0 * d.reshape(-1, 3)[hot]
                v, _ = both(pts, scan, IDENTITY, H, W, tables, p)
                hl, hc = divmod(hot, W)
                l, c = np.divmod(np.arange(H * W), W)
                dc = np.minimum((c - hc) % W, (hc - c) % W)
                reach = (np.abs(l - hl) <= wl) & (dc <= wc)
                assert np.array_equal(v == V.AGREE, reach) and np.array_equal(v == V.EMPTY, ~reach), (H, W, wl, wc, hot)
        scan = V.shell_scan(rng, H, W)
        both(pts, scan, IDENTITY, H, W, tables, V.Params(window_lines=3, window_cols=3))


def test_unusable_cells_of_each_kind_leave_the_window_empty_and_one_near_return_occludes():
    H, W = 4, 8
    tables = V.analytic_tables(H, W, FAN)
    pt = np.array([[10.0, 0.0, 0.0]])
    cell = int(V.O.classify(pt, *tables)[0][0])
    p = V.Params(window_lines=0, window_cols=0)
    for bad in ([0, 0, 0], [np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [0.5, 0.5, 0.5], [np.nextafter(1.0, 0), 0, 0]):
        scan = np.full((H * W, 3), 50.0)
        scan[cell] = bad
        assert both(pt, scan, IDENTITY, H, W, tables, p)[0][0] == V.EMPTY, bad
    for r, want in ((1.0, V.OCCLUDED), (5.0, V.OCCLUDED), (10.0, V.AGREE), (50.0, V.THROUGH), (1e200, V.THROUGH)):
        scan = np.zeros((H * W, 3))
        scan[cell] = [r, 0, 0]
        assert both(pt, scan, IDENTITY, H, W, tables, p)[0][0] == want, r
    # THROUGH needs every usable cell beyond: one nearer return in the window turns it into OCCLUDED, one agreeing into AGREE
    p = V.Params()
    scan = np.full((H * W, 3), 0.0)
    scan[:, 0] = 50.0
    assert both(pt, scan, IDENTITY, H, W, tables, p)[0][0] == V.THROUGH
    scan[cell - W] = [4.0, 0, 0]
    assert both(pt, scan, IDENTITY, H, W, tables, p)[0][0] == V.OCCLUDED
    scan[(cell + 1) % W + (cell // W) * W] = [10.2, 0, 0]
    assert both(pt, scan, IDENTITY, H, W, tables, p)[0][0] == V.AGREE


def test_the_decision_at_min_through_and_at_the_ratio_and_one_off():
    votes = np.zeros(0, dtype=V.VOTES_DTYPE)
    rows = [(t, a, 0, 0) for t in (0, 1, 2, 3, 4, 5, 7, 0xFFFFFFFF) for a in (0, 1, 2, 3, 4, 10, 0xFFFFFFFF)]
    votes = np.array(rows, dtype=V.VOTES_DTYPE)
    for p in (V.Params(), V.Params(min_through=0), V.Params(min_through=3, through_ratio=0.5), V.Params(through_ratio=1.5), V.Params(through_ratio=0.0),
              V.Params(min_through=0xFFFFFFFF), V.Params(through_ratio=1.0 / 3.0)):
        assert np.array_equal(V.header_dynamic(votes, p), V.dynamic(votes, p)), p.items()
    d = V.dynamic(np.array([(2, 2, 0, 0), (1, 0, 0, 0), (2, 3, 0, 0), (3, 3, 9, 9), (3, 2, 0, 0)], dtype=V.VOTES_DTYPE))
    assert d.tolist() == [True, False, False, True, True]  # through == min_through and == ratio agree; one short of either
    d = V.dynamic(np.array([(3, 2, 0, 0), (2, 2, 0, 0), (4, 2, 0, 0)], dtype=V.VOTES_DTYPE), V.Params(through_ratio=1.5))
    assert d.tolist() == [True, False, True]
    dyn, xyz, keep, n = V.filter_static(np.array([(2, 0, 0, 0), (0, 5, 0, 0), (9, 1, 0, 0), (1, 1, 0, 0)], dtype=V.VOTES_DTYPE), None,
                                        np.arange(12.0).reshape(4, 3), capacity=1)
    assert dyn.tolist() == [1, 0, 1, 0] and n == 2 and keep.tolist() == [1] and xyz.tolist() == [[3.0, 4.0, 5.0]]


def test_the_same_functions_are_clean_under_asan_and_ubsan_in_a_stand_alone_program():
    subprocess.check_call(["make", "-s", "-C", V.HOSTCHECK_DIR, "san"])
    out = subprocess.run([os.path.join(V.HOSTCHECK_DIR, "hostcheck_visibility_san")], capture_output=True, text=True, timeout=300)
    text = out.stdout + out.stderr
    assert out.returncode == 0 and "hostcheck_visibility ok" in out.stdout, text[-3000:]
    assert "runtime error" not in text and "AddressSanitizer" not in text, text[-3000:]
