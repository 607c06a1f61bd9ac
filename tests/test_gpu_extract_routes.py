"""GPU: the extraction kernels across their whole parameter range, against the CPU oracle by equality.

Which kernels an extraction runs depends on neighbor_points, the sector length, number_sectors, the caps, scan_lines % 4,
points_per_line % 16 and the number of scan lines in the call (extract_kernels.hip: launch_select, row_select_geom). Every
case here goes through loamx_extract_features_batch_dev with index arrays and point copies, double and float input, and is
compared per scan with oracle.extract_features: both index sequences, the counts, the copied points bit for bit. WHICH
kernels ran is read back from the library (loamx_ctx_last_extract_route, set by the launchers themselves) and asserted:
a test of "the row kernels at geometry X" fails instead of silently becoming a test of another kernel when a predicate moves.

  (a) random row-kernel geometries          (b) the accepted shapes with the least room
  (c) one step outside each shape of (b)    (d) the walls of the parameter range
  (e) the bounding boxes the row kernels hand to the index builds, through the scan-pair pipeline

Run with -s to see, per route bit, how many cases ran it."""
import collections
import contextlib

import numpy as np
import pytest

from gpu_common import ctx, option, pose_diff
from loam_amd import capi

pytestmark = pytest.mark.gpu

KINDS = ("noisy", "clean", "rounded", "dropped")
THRESHOLDS = (100.0, 1.0, 0.5, 1.0)  # edge, planar, occlusion, parallel: the reference's defaults

_TALLY = collections.Counter()  # route bit / selection kernel -> cases of this module that ran it


@pytest.fixture(scope="module", autouse=True)
def _print_tally():
    yield
    print("\nextraction routes taken by the cases of this module (cases per route bit):")
    for name, n in sorted(_TALLY.items()):
        print("  %-16s %5d" % (name, n))


def make_scans(seed, H, W, n_scans, kind):
    """n_scans scans of one kind: sigma = 0.01 noise; noise free (exact curvature ties, hence the std::sort replay);
    rounded to 1/32 m (a fixed-point sensor: ties in every sector); 5 % of the points zeroed (drop-outs)."""
    sigma = 0.0 if kind == "clean" else 0.01
    scans = np.stack([capi.synth_scan_host(seed + s, s % 5, s & 1, H, W, sigma) for s in range(n_scans)])
    if kind == "rounded":
        scans = np.round(scans * 32.0) / 32.0
    if kind == "dropped":
        scans[np.random.default_rng(seed).random(scans.shape[:2]) < 0.05] = 0.0
    return np.ascontiguousarray(scans)


def selection(route):
    """the selection kernel a route word names, as one label"""
    if "ROWS" in route:
        return "ROWS"
    if "MIS" in route:
        return "MIS%d%s" % (4 if "MIS_4LINES" in route else 1, "_TWO" if "MIS_TWO" in route else "")
    return "ARGMAX4" if "ARGMAX4" in route else "ARGMAX1" if "ARGMAX1" in route else "NONE"


def run_case(oracle, H, W, params, scans, f32=False, options=(), tag=None):
    """One batched extraction of `scans` ([n_scans][H * W][3] doubles; f32: narrowed first, and the oracle works on the
    widened scan, as the reference's FieldAccessor does) under the given context options: everything against the oracle,
    scan by scan. Returns the route the library reports for the call."""
    c = ctx()
    ns = len(scans)
    data = np.ascontiguousarray(scans.astype(np.float32)) if f32 else scans
    wide = data.astype(np.float64)
    lidar, fe, ofe = capi.LidarParams(H, W, 1.0, 120.0), capi.FeatureExtractionParams(*params), oracle.FeParams(*params)
    ecap, pcap = c.edge_capacity(lidar, fe), c.planar_capacity(lidar, fe)
    bufs = [c.alloc(data.nbytes).upload(data)]
    bufs += [c.alloc(ns * ecap * 4), c.alloc(ns * 4), c.alloc(ns * ecap * 24), c.alloc(ns * pcap * 4), c.alloc(ns * 4), c.alloc(ns * pcap * 24)]
    d_xyz, d_ei, d_ne, d_ex, d_pi, d_np, d_px = bufs
    try:
        with contextlib.ExitStack() as stack:
            for o in options:
                stack.enter_context(option(o))
            c.extract_features_batch_dev(d_xyz.ptr, ns, lidar, fe, d_ei.ptr, d_ne.ptr, d_ex.ptr, d_pi.ptr, d_np.ptr, d_px.ptr, f32=f32)
            c.synchronize()
            route = c.last_extract_route()
        ne, npl = d_ne.download(np.uint32, ns), d_np.download(np.uint32, ns)
        ei = d_ei.download(np.uint32, ns * ecap).reshape(ns, ecap)
        pi = d_pi.download(np.uint32, ns * pcap).reshape(ns, pcap)
        ex = d_ex.download(np.float64, ns * ecap * 3).reshape(ns, ecap, 3)
        px = d_px.download(np.float64, ns * pcap * 3).reshape(ns, pcap, 3)
    finally:
        for b in bufs:
            b.free()
    what = (tag, H, W, params, ns, "f32" if f32 else "f64", options, route)
    for s in range(ns):
        oe, op = oracle.extract_features(wide[s], H, W, 1.0, 120.0, ofe)
        assert (ne[s], npl[s]) == (len(oe), len(op)), (what, s)
        assert np.array_equal(ei[s, :ne[s]], oe), (what, s)
        assert np.array_equal(pi[s, :npl[s]], op), (what, s)
        assert np.array_equal(ex[s, :ne[s]].view(np.uint64), wide[s][oe].view(np.uint64)), (what, s)
        assert np.array_equal(px[s, :npl[s]].view(np.uint64), wide[s][op].view(np.uint64)), (what, s)
    for name in route.names:
        _TALLY[name] += 1
    _TALLY["select:" + selection(route)] += 1
    return route


def run_both(oracle, H, W, params, scans, options=(), tag=None):
    """double and float input; the route does not depend on the scalar type"""
    r64 = run_case(oracle, H, W, params, scans, False, options, tag)
    r32 = run_case(oracle, H, W, params, scans, True, options, tag)
    assert r64.bits == r32.bits, (tag, r64, r32)
    return r64


# ---- (a) row-kernel geometry, random -----------------------------------------------------------------------------------
A_DRAWS, A_GROUPS = 400, 8


def draw_a(i):
    """draw i of the generator: neighbor_points 2..5 (R = np - 1), 1..16 sectors of L points, L uniform from the shortest
    line the reference accepts to just past the longest sector the row kernels take (64 picks R + 1 apart), the line
    rounded up to the 16 columns they ask for, 4..20 lines (multiples of four), caps on either side of the 64 kept picks,
    thresholds as in test_extraction_fuzz_against_the_oracle, 1..5 scans (so that the lines of a call leave 0, 4, 8 or 12
    in its last workgroup of 16 and most calls span several workgroups)."""
    rng = np.random.default_rng(91000 + i)
    np_ = int(rng.integers(2, 6))
    R = np_ - 1
    S = int(rng.integers(1, 17))
    L = int(rng.integers(2 * np_ + 2, 64 * (R + 1) - R + 12))
    W = min((L * S + 15) // 16 * 16, 4096)
    H = int(rng.choice([4, 8, 12, 20]))
    max_edge = int(rng.choice([0, 1, 5, 10, 30, 63, 64, 100]))
    max_planar = int(rng.choice([0, 3, 20, 50, 63, 64, 200]))
    params = (np_, S, max_edge, max_planar, float(rng.choice([5.0, 50.0, 100.0, 1e4])), float(rng.choice([0.05, 1.0, 20.0])),
              float(rng.choice([0.1, 0.5])), float(rng.choice([0.02, 1.0])))
    return H, W, params, int(rng.integers(1, 6)), KINDS[int(rng.integers(0, 4))], int(rng.integers(1, 1000))


_A_SEEN = {}  # group -> [(H, W, params, n_scans, route)]


def run_a_group(oracle, g):
    if g not in _A_SEEN:
        seen = []
        for i in range(g, A_DRAWS, A_GROUPS):
            H, W, params, ns, kind, seed = draw_a(i)
            assert W >= 2 * params[0] + 2
            route = run_both(oracle, H, W, params, make_scans(seed, H, W, ns, kind), tag=("a", i, kind))
            seen.append((H, W, params, ns, route))
        _A_SEEN[g] = seen
    return _A_SEEN[g]


@pytest.mark.parametrize("group", range(A_GROUPS))
def test_a_random_row_geometries_against_the_oracle(oracle, group):
    """400 draws in 8 groups; whichever kernels a draw selects, the result is the oracle's"""
    run_a_group(oracle, group)


def test_a_random_row_geometries_cover_the_row_kernels(oracle):
    """What the 400 draws reached, counted from the library's own route readout (groups not run yet are run here):
    at least 200 calls of select_rows_kernel, every R, both pick-list widths, at least 30 (R, points per lane) pairs, the
    instantiation specialised for 11 points per lane and the generic one, lines that do not divide into their sectors and
    a cap above the 64 picks the kernel keeps."""
    seen = [x for g in range(A_GROUPS) for x in run_a_group(oracle, g)]
    rows = [x for x in seen if "ROWS" in x[4]]
    print("\n(a): %d of %d draws took the row kernels; others: %s" % (len(rows), len(seen), dict(collections.Counter(selection(x[4]) for x in seen if "ROWS" not in x[4]))))
    pairs = sorted({(x[4].rows_R, x[4].rows_ch) for x in rows})
    print("(a): (R, ch) pairs:", pairs)
    assert len(rows) >= 200
    assert {r for r, _ in pairs} == {1, 2, 3, 4}
    assert all(x[4].rows_R == x[2][0] - 1 for x in rows)
    assert {"ROWS_LIST16" in x[4] for x in rows} == {False, True}
    assert len(pairs) >= 30
    assert {"ROWS_CH11" in x[4] for x in rows} == {False, True}
    assert any(W % params[1] != 0 for _, W, params, _, _ in rows)

    def cap(W, S, most):  # entries of a sector's slot (loamx_edge_capacity / H / S): min(max + 1, longest sector)
        return min(most + 1, W - (S - 1) * (W // S))
    assert any(max(cap(W, p[1], p[2]), cap(W, p[1], p[3])) > 64 for _, W, p, _, _ in rows)
    assert {(ns * H) % 16 for H, _, _, ns, _ in rows} == {0, 4, 8, 12}
    assert sum(ns * H > 16 for H, _, _, ns, _ in rows) > len(rows) // 2  # more than one workgroup


# ---- (b) row-kernel geometry at the predicate's edges ------------------------------------------------------------------
# (neighbor_points, W, number_sectors, max_edge, max_planar). row_select_geom lets a shape in when, among other bounds, the
# copy phase's buffers fit below the slot lists (slack = off_sl - (24 * longest + 1536) >= 0), a wavefront's LDS block is at
# most 16 KB and a sector yields at most 64 picks; these are the accepted shapes with the least room. Every one is confirmed
# to run select_rows_kernel by the route readout (none had to be replaced).
B_SLACK0 = [(2, 400, 4, 10, 50), (3, 416, 5, 10, 50), (4, 80, 1, 10, 50), (5, 256, 6, 10, 50), (2, 736, 13, 10, 50), (3, 720, 15, 10, 50),
            (4, 496, 11, 10, 50)]  # copy-phase slack exactly 0
B_LDS = [(5, 2576, 11, 63, 63), (4, 2640, 12, 63, 63), (3, 2608, 14, 63, 63), (2, 2048, 16, 63, 63)]  # LDS block = / next to 16 384 B
B_LONG = [(2, 128, 1, 10, 50), (3, 192, 1, 10, 50), (4, 256, 1, 10, 50), (5, 320, 1, 10, 50),  # one sector of 64 picks
          (5, 1584, 5, 10, 50),   # 21 points per lane (the most), 16-bit lists
          (4, 2240, 9, 10, 50),   # 17 points per lane, 16-bit lists
          (3, 3056, 16, 10, 50),  # longest sector 191 = 64 picks
          (4, 4048, 16, 10, 50), (5, 4032, 16, 10, 50)]
B_SHAPES = B_SLACK0 + B_LDS + B_LONG
B_H, B_SCANS = 8, 3  # 24 lines: two workgroups, the second half empty


def shape_id(s):
    return "np%d-W%d-S%d" % s[:3]


@pytest.mark.parametrize("shape", B_SHAPES, ids=shape_id)
def test_b_edge_shapes_run_the_row_kernels(oracle, shape):
    np_, W, S, me, mp = shape
    for k, kind in enumerate(KINDS):
        route = run_both(oracle, B_H, W, (np_, S, me, mp) + THRESHOLDS, make_scans(700 + k, B_H, W, B_SCANS, kind), tag=("b", kind))
        assert "ROWS" in route and route.rows_R == np_ - 1, route
        assert "FUSED_COMPACT" in route and "ROWS_PASS2" in route, route
    expect = {(5, 1584, 5): (21, True), (4, 2240, 9): (17, True), (5, 320, 1): (21, True), (4, 256, 1): (17, True), (3, 3056, 16): (13, False)}
    if shape[:3] in expect:
        assert (route.rows_ch, "ROWS_LIST16" in route) == expect[shape[:3]], route


@pytest.mark.parametrize("forced", ["FORCE_TIE_REPLAY", "FORCE_SCAN_GIVEUP", "NO_FUSED_COMPACT", "NO_SPLIT_CURV", "STAGE_ALWAYS"])
@pytest.mark.parametrize("shape", B_SLACK0, ids=shape_id)
def test_b_slack0_shapes_with_the_rare_paths_forced(oracle, shape, forced):
    """the copy phase reuses the curvature buffer to its last byte on these shapes: every line through the std::sort replay,
    every scan through the fallback compaction, the separate compaction, the stage arrays written by the first launch —
    the oracle's results, and the counters move as in test_forced_replay_and_forced_fallback_change_nothing"""
    np_, W, S, me, mp = shape
    params = (np_, S, me, mp) + THRESHOLDS
    scans = make_scans(750, B_H, W, B_SCANS, "noisy")
    c = ctx()
    for f32 in (False, True):
        r0, f0 = c.extract_counters()
        plain = run_case(oracle, B_H, W, params, scans, f32)
        assert c.extract_counters() == (r0, f0)  # noisy scans: neither rare path ran
        route = run_case(oracle, B_H, W, params, scans, f32, (forced,), tag="b-forced")
        r1, f1 = c.extract_counters()
        assert "ROWS" in plain and "ROWS" in route and (route.rows_R, route.rows_ch) == (plain.rows_R, plain.rows_ch), (plain, route)
        if forced == "FORCE_TIE_REPLAY":
            assert r1 - r0 == B_SCANS * B_H
        elif forced == "FORCE_SCAN_GIVEUP":
            assert (r1 - r0, f1 - f0) == (0, 1)
        else:
            assert (r1, f1) == (r0, f0)
        if forced == "NO_FUSED_COMPACT":
            assert "COMPACT" in route and "FUSED_COMPACT" not in route and "ROWS_PASS2" not in route, route
        if forced == "STAGE_ALWAYS":
            assert "FUSED_COMPACT" in route and "ROWS_PASS2" not in route, route
        if forced == "NO_SPLIT_CURV":
            assert "SPLIT_CURV" not in route, route


# ---- (c) one step outside ----------------------------------------------------------------------------------------------
# 16 more columns push these shapes of (b) over a bound (65 picks, negative slack, an LDS block above 16 KB); the other
# four stay inside with 16 more
C_WIDER = [s for s in B_SHAPES if s[:3] not in {(4, 80, 1), (5, 1584, 5), (4, 2240, 9), (3, 3056, 16)}]


def outside_cases():
    for s in B_SHAPES:
        np_, W, S, me, mp = s
        yield "H6-" + shape_id(s), 6, W, (np_, S, me, mp)       # scan_lines % 4 != 0 (12 lines in the call: a multiple of four)
        yield "S17-" + shape_id(s), 8, W, (np_, 17, me, mp)     # more sectors than the lanes of a row
        yield "np6-" + shape_id(s), 8, W, (6, S, me, mp)        # R = 5
        yield "odd-" + shape_id(s), 8, W + 1, (np_, S, me, mp)  # points_per_line % 16 != 0
    for s in C_WIDER:
        np_, W, S, me, mp = s
        yield "W+16-" + shape_id(s), 8, W + 16, (np_, S, me, mp)


@pytest.mark.parametrize("name,H,W,p4", list(outside_cases()), ids=[x[0] for x in outside_cases()])
def test_c_one_condition_broken_takes_another_route(oracle, name, H, W, p4):
    for k, kind in enumerate(("noisy", "clean")):
        route = run_both(oracle, H, W, p4 + THRESHOLDS, make_scans(800 + k, H, W, 2, kind), tag=("c", name, kind))
        assert "ROWS" not in route and selection(route) != "NONE", route


def test_c_three_lines_short_of_a_multiple_of_four_in_the_call(oracle):
    """scan_lines % 4 == 0 is asked of the scan, (lines in the call) % 4 == 0 of the launch: one scan of 6 lines fails both,
    two scans of 6 lines only the first — neither may run the row kernels (test_c_... above runs the second)"""
    np_, W, S, me, mp = B_SLACK0[0]
    route = run_both(oracle, 6, W, (np_, S, me, mp) + THRESHOLDS, make_scans(810, 6, W, 1, "noisy"))
    assert "ROWS" not in route, route


# ---- (d) the walls -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("np_", range(6, 17))
def test_d_wide_halos_generic_curvature_and_arg_max(oracle, np_):
    """neighbor_points 6..16 (the library's bound): curvature_valid_kernel<0> with halos of up to 16 columns on either side,
    select_kernel<4> (lines up to 1024) / <1> (longer), the separate compaction"""
    for k, W in enumerate((40, 333, 1024, 4096)):
        H, S = (4 if W == 4096 else 5), (2 if W == 40 else 6)
        assert W >= 2 * np_ + 2
        route = run_both(oracle, H, W, (np_, S, 10, 50) + THRESHOLDS, make_scans(900 + np_, H, W, 2, KINDS[(np_ + k) % 4]), tag="d-np")
        assert selection(route) == ("ARGMAX1" if W > 1024 else "ARGMAX4"), route
        assert "CURV_GENERIC" in route and "COMPACT" in route and "FUSED_COMPACT" not in route, route


# (H, W, neighbor_points, number_sectors, max_edge, max_planar, selection kernel): long lines. One wavefront per line
# once four lines no longer fit one workgroup's LDS; two picks per lane for 65..128 picks per sector while both caps are
# at most 64; the arg-max kernel beyond (and wherever a lane's chunk + halo no longer fits 64 bits: W >= 3968 for R >= 2,
# 4096 for every R).
D_LONG_LINES = [
    (4, 2064, 2, 20, 10, 50, "MIS1"), (6, 2064, 2, 11, 10, 50, "MIS1_TWO"), (6, 2064, 2, 11, 100, 200, "ARGMAX1"),
    (4, 2064, 3, 20, 10, 50, "MIS1"), (6, 2064, 3, 7, 10, 50, "MIS1_TWO"), (6, 2064, 3, 7, 100, 200, "ARGMAX1"),
    (4, 2064, 4, 20, 10, 50, "MIS1"), (6, 2064, 4, 6, 10, 50, "MIS1_TWO"), (6, 2064, 4, 6, 100, 200, "ARGMAX1"),
    (4, 2064, 5, 20, 10, 50, "MIS1"), (6, 2064, 5, 5, 10, 50, "MIS1_TWO"), (6, 2064, 5, 5, 100, 200, "ARGMAX1"),
    (4, 3000, 2, 20, 10, 50, "MIS1_TWO"), (6, 3000, 2, 15, 10, 50, "MIS1_TWO"), (6, 3000, 2, 15, 100, 200, "ARGMAX1"),
    (4, 3000, 3, 20, 10, 50, "MIS1"), (6, 3000, 3, 10, 10, 50, "MIS1_TWO"), (6, 3000, 3, 10, 100, 200, "ARGMAX1"),
    (4, 3000, 4, 20, 10, 50, "MIS1"), (6, 3000, 4, 8, 10, 50, "MIS1_TWO"), (6, 3000, 4, 8, 100, 200, "ARGMAX1"),
    (4, 3000, 5, 20, 10, 50, "MIS1"), (6, 3000, 5, 6, 10, 50, "MIS1_TWO"), (6, 3000, 5, 6, 100, 200, "ARGMAX1"),
    (4, 3584, 2, 20, 10, 50, "MIS1_TWO"), (6, 3584, 2, 18, 10, 50, "MIS1_TWO"), (6, 3584, 2, 18, 100, 200, "ARGMAX1"),
    (4, 3584, 3, 20, 10, 50, "MIS1"), (6, 3584, 3, 12, 10, 50, "MIS1_TWO"), (6, 3584, 3, 12, 100, 200, "ARGMAX1"),
    (4, 3584, 4, 20, 10, 50, "MIS1"), (6, 3584, 4, 9, 10, 50, "MIS1_TWO"), (6, 3584, 4, 9, 100, 200, "ARGMAX1"),
    (4, 3584, 5, 20, 10, 50, "MIS1"), (6, 3584, 5, 8, 10, 50, "MIS1_TWO"), (6, 3584, 5, 8, 100, 200, "ARGMAX1"),
    (4, 3968, 2, 20, 10, 50, "MIS1_TWO"), (6, 3968, 2, 20, 63, 63, "MIS1_TWO"), (6, 3968, 2, 20, 100, 200, "ARGMAX1"),
    (4, 3968, 3, 20, 10, 50, "ARGMAX1"), (6, 3968, 4, 10, 10, 50, "ARGMAX1"), (6, 3968, 5, 8, 100, 200, "ARGMAX1"),
    (4, 4096, 2, 20, 10, 50, "ARGMAX1"), (6, 4096, 3, 14, 10, 50, "ARGMAX1"), (6, 4096, 3, 14, 100, 200, "ARGMAX1"),
    (4, 4096, 4, 20, 10, 50, "ARGMAX1"), (6, 4096, 5, 9, 10, 50, "ARGMAX1"),
]


@pytest.mark.parametrize("W", [2064, 3000, 3584, 3968, 4096])
def test_d_long_lines(oracle, W):
    for k, (H, W_, np_, S, me, mp, sel) in enumerate(x for x in D_LONG_LINES if x[1] == W):
        route = run_both(oracle, H, W, (np_, S, me, mp) + THRESHOLDS, make_scans(1000 + k, H, W, 2, KINDS[k % 4]), tag="d-long")
        assert selection(route) == sel, (route, sel)
        assert ("FUSED_COMPACT" in route) == (sel.startswith("MIS") and S <= 64), route  # (the arg-max kernel never writes the final arrays)
        assert ("CURV2" in route) == (np_ == 3) and ("CURV_GENERIC" in route) == (np_ != 3), route


# (H, W, neighbor_points, number_sectors, max_edge, max_planar, selection kernel): many sectors — the fused compaction keeps
# a line's sector counts on the 64 lanes of a wavefront, beyond that compact_kernel gathers — up to more sectors than points
# (points per sector 0: everything falls into the last sector), and caps of 0 and 1000
D_SECTORS_CAPS = [
    (4, 256, 3, 17, 10, 50, "MIS4"), (4, 256, 3, 64, 10, 50, "MIS4"), (4, 256, 3, 65, 10, 50, "MIS4"), (4, 256, 3, 300, 10, 50, "MIS4_TWO"),
    (4, 256, 3, 261, 10, 50, "MIS4_TWO"), (4, 256, 3, 6, 0, 0, "MIS4"), (4, 256, 3, 6, 1000, 1000, "MIS4"), (4, 256, 3, 6, 0, 1000, "MIS4"),
    (4, 256, 3, 65, 0, 0, "MIS4"), (4, 256, 3, 65, 1000, 1000, "MIS4"), (4, 256, 3, 65, 0, 1000, "MIS4"),
    (4, 1024, 2, 17, 10, 50, "MIS4"), (4, 1024, 2, 64, 10, 50, "MIS4"), (4, 1024, 2, 65, 10, 50, "MIS4"), (4, 1024, 2, 300, 10, 50, "MIS4"),
    (4, 1024, 2, 1029, 10, 50, "ARGMAX4"), (4, 1024, 2, 6, 0, 0, "MIS4_TWO"), (4, 1024, 2, 6, 1000, 1000, "ARGMAX4"),
    (4, 1024, 2, 6, 0, 1000, "ARGMAX4"), (4, 1024, 2, 65, 0, 0, "MIS4"), (4, 1024, 2, 65, 1000, 1000, "MIS4"), (4, 1024, 2, 65, 0, 1000, "MIS4"),
    # four lines per workgroup, one and two picks per lane, with and without the line length compiled in; rows with caps 0 / 1000
    (5, 1000, 3, 6, 10, 50, "MIS4"), (5, 1000, 3, 3, 10, 50, "MIS4_TWO"), (6, 1024, 3, 6, 10, 50, "MIS4"), (4, 1024, 3, 3, 10, 50, "MIS4_TWO"),
    (4, 1024, 3, 6, 0, 0, "ROWS"), (4, 1024, 3, 6, 1000, 1000, "ROWS"), (4, 1024, 3, 16, 0, 1000, "ROWS"),
]


@pytest.mark.parametrize("part", range(4))
def test_d_many_sectors_and_extreme_caps(oracle, part):
    for k, (H, W, np_, S, me, mp, sel) in enumerate(D_SECTORS_CAPS):
        if k % 4 != part:
            continue
        assert H * S * (max(me, mp) + 1) < 1 << 22  # (the oracle binding allocates that many indices)
        route = run_both(oracle, H, W, (np_, S, me, mp) + THRESHOLDS, make_scans(1100 + k, H, W, 2, KINDS[(k // 4) % 4]), tag="d-sectors")
        assert selection(route) == sel, (route, sel, (H, W, np_, S, me, mp))
        assert ("FUSED_COMPACT" in route) == (sel != "ARGMAX4" and S <= 64), route
        assert ("COMPACT" in route) == (sel == "ARGMAX4" or S > 64), route
        if (H, W, np_, S) == (6, 1024, 3, 6):
            assert "MIS_CONST_W" in route, route


def test_d_the_walls_were_reached(oracle):
    """every kernel family of the list ran in the cases above (the tables name the kernel per case and each case asserts
    it from the readout; this is the list itself, so that a row cannot be dropped unnoticed)"""
    want = {"MIS4", "MIS4_TWO", "MIS1", "MIS1_TWO", "ARGMAX4", "ARGMAX1", "ROWS"}
    assert {x[6] for x in D_LONG_LINES + D_SECTORS_CAPS} == want
    assert any(x[3] > 64 and x[6].startswith("MIS") for x in D_SECTORS_CAPS)  # separate compaction behind a MIS selection
    assert any(x[3] > x[1] for x in D_SECTORS_CAPS)  # points per sector 0
    assert {x[2] for x in D_LONG_LINES if x[6] == "MIS1"} == {2, 3, 4, 5} and {x[2] for x in D_LONG_LINES if x[6] == "MIS1_TWO"} == {2, 3, 4, 5}


@pytest.mark.parametrize("opt,names", [("CURV_V1", {"CURV_V1", "ROWS", "ROWS_CH11", "ROWS_PASS2", "FUSED_COMPACT"}),
                                       ("FUSED_EXTRACT", {"FUSED_EXTRACT", "FUSED_COMPACT"}),
                                       ("FUSED_ROWS", {"FUSED_ROWS", "ROWS", "ROWS_CH11", "FUSED_COMPACT"})], ids=lambda x: x if isinstance(x, str) else "")
def test_d_opt_in_kernels(oracle, opt, names):
    """the kernels only an option selects, on the default parameters: the one-column curvature kernel, the one-pass
    extraction kernel, the fused form of the row kernels — all four kinds of input"""
    H, W = 8, 1024
    for k, kind in enumerate(KINDS):
        route = run_both(oracle, H, W, (3, 6, 10, 50) + THRESHOLDS, make_scans(1200 + k, H, W, 2, kind), (opt,), tag="d-" + opt)
        assert route.names == names, route


def test_default_parameters_take_the_specialised_row_kernels(oracle):
    """the default route, as the readout names it: split curvature hand-over from curvature_valid2_kernel to
    select_rows_kernel<2, 11>, fused compaction, the conditional second pass"""
    H, W = 8, 1024
    route = run_both(oracle, H, W, (3, 6, 10, 50) + THRESHOLDS, make_scans(1300, H, W, 3, "noisy"))
    assert route.names == {"SPLIT_CURV", "CURV2", "ROWS", "ROWS_CH11", "ROWS_PASS2", "FUSED_COMPACT"}, route
    assert (route.rows_R, route.rows_ch) == (2, 11)
    route = run_both(oracle, H, W, (3, 6, 10, 50) + THRESHOLDS, make_scans(1300, H, W, 3, "noisy"), ("NO_SPLIT_CURV",))
    assert route.names == {"CURV2", "ROWS", "ROWS_CH11", "ROWS_PASS2", "FUSED_COMPACT"}, route
    route = run_both(oracle, H, W, (3, 6, 10, 50) + THRESHOLDS, make_scans(1300, H, W, 3, "noisy"), ("NO_ROW_SELECT",))
    assert route.names == {"CURV2", "MIS", "MIS_4LINES", "MIS_CONST_W", "FUSED_COMPACT"}, route
    route = run_both(oracle, H, W, (3, 6, 10, 50) + THRESHOLDS, make_scans(1300, H, W, 3, "noisy"), ("NO_MIS_SELECT",))
    assert route.names == {"CURV2", "ARGMAX4", "COMPACT"}, route


# ---- (e) boxes into the pipeline ---------------------------------------------------------------------------------------
# (scan lines, neighbor_points, W, number_sectors, max_edge, max_planar): the default geometry, a slack-0 shape, the full
# LDS block, 16-bit lists at 17 points per lane, 16 sectors of 64 picks
E_GEOMETRIES = [(16, 3, 1024, 6, 10, 50), (20, 2, 400, 4, 10, 50), (16, 5, 2576, 11, 63, 63), (16, 4, 2240, 9, 10, 50), (16, 3, 3056, 16, 10, 50)]


@pytest.mark.parametrize("geometry", E_GEOMETRIES, ids=lambda g: "H%d-np%d-W%d-S%d" % g[:4])
def test_e_row_kernel_boxes_through_the_scan_pair_pipeline(oracle, geometry):
    """select_rows_kernel takes the bounding boxes of the feature sets in its copy phase and the index builds use them in
    place of a read pass of their own: the results with them equal, byte for byte, those with the builds' own boxes
    (NO_EXTRACT_BOXES), and one pair meets the oracle as in test_gpu_shapes.py"""
    H, np_, W, S, me, mp = geometry
    P, N, seed, first = 4, H * W, 515151, 3
    c = ctx()
    lidar, reg, oreg = capi.LidarParams(H, W, 1.0, 120.0), capi.RegistrationParams(), oracle.RegParams()
    params = (np_, S, me, mp) + THRESHOLDS
    fe, ofe = capi.FeatureExtractionParams(*params), oracle.FeParams(*params)
    d_xyz, d_res = c.alloc(P * 2 * N * 24), c.alloc(P * 64)
    c.synth_scan_pairs_dev(seed, first, P, H, W, 0.01, d_xyz.ptr)
    runs = {}
    for boxes in (True, False):
        with option("NO_EXTRACT_BOXES", 0 if boxes else 1):
            c.register_scan_pairs_dev(d_xyz.ptr, P, lidar, fe, reg, d_res.ptr)
            c.synchronize()
            route = c.last_extract_route()
        assert "ROWS" in route and "FUSED_COMPACT" in route and route.rows_R == np_ - 1, route
        if boxes:
            assert "BOXES" in route, route
        runs[boxes] = d_res.download(np.uint8, P * 64).copy()
    d_xyz.free()
    d_res.free()
    assert np.array_equal(runs[True], runs[False])
    res = runs[True].view(capi.RESULT_DTYPE)
    pr = 1
    A = capi.synth_scan_host(seed, first + pr, 0, H, W, 0.01)
    B = capi.synth_scan_host(seed, first + pr, 1, H, W, 0.01)
    ea, pa = oracle.extract_features(A, H, W, 1.0, 120.0, ofe)
    eb, pb = oracle.extract_features(B, H, W, 1.0, 120.0, ofe)
    po, to, io = oracle.register_features(B[eb], B[pb], A[ea], A[pa], None, oreg)
    assert (res[pr]["termination"], res[pr]["iterations"]) == (to, io)
    rot, trans = pose_diff(oracle, po, res[pr]["pose"])
    print("\n(e) %s: %d / %d edge, %d / %d planar features, termination %d after %d iterations, rot %.2e trans %.2e" %
          (geometry, len(eb), len(ea), len(pb), len(pa), to, io, rot, trans))
    assert rot < 1e-5 and trans < 1e-5, (to, rot, trans)
