"""GPU: loamx_segment_scans_dev[_f32] / loamx_segment_scan[_f32] (include/loamx.h, "scan segmentation") against the numpy model
of tests/segment_common.py, by equality on every cell of every output: classes, labels, sizes, the filtered scan (compared as
bits), the cluster table and the stats. Output buffers are poisoned before every call. The tile form and the global-only form
(context option NO_SEGMENT_TILES) must give the same bytes, and the census of edges handed to the global union must be the
model's for either form."""
import ctypes as C
import itertools

import numpy as np
import pytest

import segment_common as M
from gpu_common import ctx, option
from loam_amd import capi

pytestmark = pytest.mark.gpu

POISON = 0xA5
OUTPUTS = ("classes", "labels", "sizes", "filtered", "clusters", "stats")
SMALL_SHAPES = [(1, 16), (2, 16), (5, 37), (8, 37), (2, 4096)]


def lidar_of(H, W):
    return capi.LidarParams(H, W, 1.0, 120.0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def tile_shape():
    c = ctx()
    c.segment_scan(np.zeros((16, 3)), lidar_of(1, 16))
    cen = c.last_segment_census()
    return cen.tile_lines, cen.tile_cols


def multi_tile_shape():
    """at least 2 x 3 tiles, neither dimension a multiple of the tile"""
    tl, tc = tile_shape()
    return tl + 5, 2 * tc + 44


def run_dev(scans, H, W, params=None, want=OUTPUTS, max_clusters=None, in_place=False, lidar=None, n_scans=None, null_scans=False, expect=None):
    """The device entry point on poisoned outputs. scans: (n, H W, 3) float64 or float32. Returns ({name: array per batch},
    census); outputs not in `want` are passed as NULL. expect: the status a refusal must give; every output must then still be
    poison."""
    c = ctx()
    scans = np.ascontiguousarray(scans)
    n, HW, dt = (len(scans) if n_scans is None else n_scans), H * W, scans.dtype
    cap = HW if max_clusters is None else max_clusters
    shapes = dict(classes=(np.uint8, n * HW), labels=(np.uint32, n * HW), sizes=(np.uint32, n * HW), filtered=(dt, n * HW * 3),
                  clusters=(capi.SEGMENT_CLUSTER_DTYPE, n * cap), stats=(np.uint32, n * 8))
    bufs = {"scans": c.alloc(max(scans.nbytes, 8))}
    for name in want:
        if not (in_place and name == "filtered"):
            bufs[name] = c.alloc(max(np.dtype(shapes[name][0]).itemsize * shapes[name][1], 8))
    try:
        bufs["scans"].upload(scans)
        for name, b in bufs.items():
            if name != "scans":
                b.upload(np.full(b.nbytes, POISON, np.uint8))
        ptr = {name: (bufs["scans"].ptr if in_place and name == "filtered" else bufs[name].ptr) if name in want else 0 for name in OUTPUTS}
        call = lambda: c.segment_scans_dev(0 if null_scans else bufs["scans"].ptr, n, lidar or lidar_of(H, W), params, ptr["classes"], ptr["labels"],
                                           ptr["sizes"], ptr["filtered"], ptr["clusters"], cap, ptr["stats"], f32=dt == np.float32)
        if expect is not None:
            with pytest.raises(capi.LoamxError) as e:
                call()
            assert e.value.status == expect, (e.value.status, str(e.value))
            c.synchronize()
            for name, b in bufs.items():
                if name != "scans":
                    assert (b.download(np.uint8, b.nbytes) == POISON).all(), name
            assert np.array_equal(bits(bufs["scans"].download(dt, scans.size)), bits(scans.reshape(-1)))
            return None, None
        call()
        c.synchronize()
        out = {}
        for name in want:
            src = bufs["scans"] if in_place and name == "filtered" else bufs[name]
            a = src.download(*shapes[name])
            out[name] = a.reshape((n, HW, 3) if name == "filtered" else (n, -1))
        return out, c.last_segment_census()
    finally:
        for b in bufs.values():
            b.free()


def same(out, i, want, where):
    """every output of scan i of a device call against a model Segmentation, by equality on every cell"""
    for name in out:
        w = getattr(want, name)
        g = out[name][i]
        if name == "clusters":
            n = len(w)
            assert (g[n:].view(np.uint8) == POISON).all(), (where, "records beyond the written ones were touched")
            g = g[:n]
        if name == "filtered":
            assert g.dtype == w.dtype, (where, g.dtype, w.dtype)
            bad = np.flatnonzero((bits(g) != bits(w)).any(axis=1))
        else:
            bad = np.flatnonzero(g != w)
        assert g.shape == w.shape and not len(bad), (where, name, len(bad), bad[:6].tolist(), g[bad[:6]].tolist(), w[bad[:6]].tolist())


def check(scans, H, W, params=None, where="", forms=(0, 1), max_clusters=None):
    """both forms on a batch against the model of every scan; returns (models, census per form)"""
    scans = np.ascontiguousarray(scans)
    if scans.ndim == 2:
        scans = scans[None]
    models = [M.segment(s, H, W, params=params, max_clusters=max_clusters) for s in scans]
    census = {}
    for no_tiles in forms:
        with option("NO_SEGMENT_TILES", no_tiles):
            out, cen = run_dev(scans, H, W, params, max_clusters=max_clusters)
        for i, m in enumerate(models):
            same(out, i, m, (where, "global-only" if no_tiles else "tiles", i))
        assert cen.tiles == (not no_tiles), (where, cen)
        assert cen.tiles_per_scan == -(-H // cen.tile_lines) * -(-W // cen.tile_cols)
        assert cen.merged_edges == sum(M.merged_edges(m, cen.tile_lines, cen.tile_cols, cen.tiles) for m in models), (where, no_tiles, cen)
        census[no_tiles] = cen
    return models, census


def mask_params(**kw):
    return capi.SegmentParams(**dict(M.MASK_PARAMS, **kw))


def mask_scenes(H, W):
    yield "random / 20 m", M.mask_scan(M.random_mask(H, W, 1))
    yield "random / invalid", M.mask_scan(M.random_mask(H, W, 2), far=None)
    yield "serpentine", M.mask_scan(M.serpentine(H, W))
    yield "comb", M.mask_scan(M.comb(H, W))
    yield "alternating lines", M.mask_scan(M.alternating_lines(H, W))
    yield "one range", M.mask_scan(np.ones((H, W), bool))
    yield "checkerboard", M.mask_scan(M.checkerboard(H, W))
    yield "all invalid", np.zeros((H * W, 3))


@pytest.mark.parametrize("H,W", SMALL_SHAPES + [(0, 0)])
def test_mask_scenes_equal_the_model_in_both_forms(H, W):
    if H == 0:  # (the multi-tile shape, read from the census)
        H, W = multi_tile_shape()
    names, scans = zip(*mask_scenes(H, W))
    models, census = check(np.stack(scans), H, W, mask_params(), where=(H, W, names))
    by = dict(zip(names, models))
    HW = H * W
    one = by["one range"]
    assert one.stats[4] + one.stats[5] == 1 and one.labels.max() == 0 and one.sizes.min() == HW
    alt = by["alternating lines"]
    assert alt.stats[4] + alt.stats[5] == H and set(alt.sizes.tolist()) == {W}
    if W % 2 == 0:
        cb = by["checkerboard"]
        assert cb.stats[3] == HW and cb.stats[6] == 1 and not cb.filtered.any()
    assert by["all invalid"].stats[0] == HW
    if H >= 3:
        sp = by["serpentine"]
        assert int(np.count_nonzero(sp.sizes == sp.sizes.max())) == int(M.serpentine(H, W).sum())  # ONE component holds the whole mask


def test_floor_under_a_downward_fan_is_all_ground():
    for H, W in ((5, 37), multi_tile_shape()):
        models, _ = check(M.floor_scan(H, W), H, W, where=("floor", H, W))
        assert models[0].stats[1] == H * W and models[0].stats[4] + models[0].stats[5] == 0


def test_tile_form_hands_fewer_edges_to_the_global_union():
    H, W = multi_tile_shape()
    for name, mask in (("serpentine", M.serpentine(H, W)), ("random", M.random_mask(H, W, 3))):
        _, census = check(M.mask_scan(mask), H, W, mask_params(), where=name)
        assert 0 < census[0].merged_edges < census[1].merged_edges, (name, census)


def test_accept_rule_at_its_edges():
    H, W = 8, 80
    m = np.zeros((H, W), bool)
    m[0, 0:29] = True                                  # 29 cells on one line: rejected
    m[2, 0:30] = True                                  # 30 cells on one line: accepted
    m[4:7, 40], m[4, 41] = True, True                  # 4 cells over 3 lines: rejected
    m[4:7, 50], m[4:6, 51] = True, True                # 5 cells over 3 lines: accepted
    m[4, 60:63], m[5, 60:62] = True, True              # 5 cells over 2 lines: rejected
    models, _ = check(M.mask_scan(m, far=None), H, W, mask_params(), where="accept rule")
    cls = models[0].classes.reshape(H, W)
    assert (cls[0, 0:29] == capi.SEGMENT_OUTLIER).all() and (cls[2, 0:30] == capi.SEGMENT_CLUSTER).all()
    assert cls[4, 40] == capi.SEGMENT_OUTLIER and cls[6, 50] == capi.SEGMENT_CLUSTER and cls[4, 61] == capi.SEGMENT_OUTLIER
    assert models[0].stats[4] == 2 and models[0].stats[5] == 3
    assert models[0].clusters.tolist() == [(2 * W, 30, 2, 2), (4 * W + 50, 5, 4, 6)]


def test_ground_lines_at_its_edges():
    H, W = 6, 40
    scan = M.floor_scan(H, W)
    for g, n_ground in ((1, 0), (2, 2 * W), (H, H * W), (H + 7, H * W), (0, H * W)):
        models, _ = check(scan, H, W, capi.SegmentParams(ground_lines=g), where=("ground_lines", g))
        assert models[0].stats[1] == n_ground, (g, models[0].stats)
    # a ground pair at the last allowed line only: a step everywhere else
    step = scan.reshape(H, W, 3).copy()
    step[:H - 2, :, 2] += 3.0 * (np.arange(H - 2) + 1.0)[:, None]
    models, _ = check(step.reshape(-1, 3), H, W, capi.SegmentParams(ground_lines=H), where="last pair")
    assert (models[0].classes.reshape(H, W)[H - 2:] == capi.SEGMENT_GROUND).all() and models[0].stats[1] == 2 * W
    models, _ = check(step.reshape(-1, 3), H, W, capi.SegmentParams(ground_lines=H - 1), where="last pair left out")
    assert models[0].stats[1] == 0


@pytest.mark.parametrize("name", ("canyon", "lot", "field"))
def test_real_scenes_f64_and_f32(name):
    H, W = 32, 512
    scan = M.real_scan(name)
    models, _ = check(scan, H, W, where=name)
    assert models[0].stats[4] >= 50 and models[0].stats[5] >= 20
    s32 = scan.astype(np.float32)
    m32, _ = check(s32, H, W, where=name + " f32")  # (the model widens; the filtered scan is compared as float32 bits)
    assert m32[0].filtered.dtype == np.float32
    # host forms
    for s, m in ((scan, models[0]), (s32, m32[0])):
        got = ctx().segment_scan(s, lidar_of(H, W))
        same({k: [v] for k, v in zip(OUTPUTS, got)}, 0, m, name + " host")


def test_real_scene_whose_components_cross_tile_borders():
    """at 64 x 1024 the lot's walls and cars span the borders of the 4 x 4 tiles: the border merge decides real components"""
    H, W = 64, 1024
    models, census = check(M.real_scan("lot", H, W), H, W, where="lot 64 x 1024")
    assert census[0].tiles_per_scan >= 4 and 0 < census[0].merged_edges < census[1].merged_edges, census
    tl = census[0].tile_lines
    rec = models[0].clusters
    assert (rec["line_max"] // tl > rec["line_min"] // tl).any(), "no accepted component spans two rows of tiles"


def test_drop_switches():
    H, W = 8, 37
    scan = M.real_scan("lot", 8, 37)
    for do, dg in itertools.product((0, 1), (0, 1)):
        check(scan, H, W, capi.SegmentParams(drop_outliers=do, drop_ground=dg, min_cluster_points=6), where=("drop", do, dg))


five_scans = M.five_scans


def test_a_batch_equals_single_calls_and_two_runs_give_the_same_bytes():
    H, W = 21, 300
    scans = five_scans(H, W)
    batch, _ = run_dev(scans, H, W)
    again, _ = run_dev(scans, H, W)
    for name in OUTPUTS:
        assert np.array_equal(batch[name].view(np.uint8), again[name].view(np.uint8)), name
    for i in range(len(scans)):
        single, _ = run_dev(scans[i:i + 1], H, W)
        for name in OUTPUTS:
            assert np.array_equal(batch[name][i].view(np.uint8), single[name][0].view(np.uint8)), (i, name)
        same(batch, i, M.segment(scans[i], H, W), ("batch", i))


@pytest.mark.parametrize("dtype", (np.float64, np.float32))
def test_filtered_in_place_equals_out_of_place(dtype):
    H, W = 21, 300
    scans = five_scans(H, W).astype(dtype)
    a, _ = run_dev(scans, H, W)
    b, _ = run_dev(scans, H, W, in_place=True)
    for name in OUTPUTS:
        assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), name


def test_null_outputs_in_every_combination():
    H, W = 8, 37
    scans = np.stack([M.real_scan("lot", H, W), M.mask_scan(M.random_mask(H, W, 9))])
    params = capi.SegmentParams(min_cluster_points=6)
    full, _ = run_dev(scans, H, W, params)
    for k in range(len(OUTPUTS) + 1):
        for want in itertools.combinations(OUTPUTS, k):
            out, _ = run_dev(scans, H, W, params, want=want)
            for name in want:
                if name == "stats" and "clusters" not in want:  # (no table: no records written)
                    assert (out[name][:, 7] == 0).all() and np.array_equal(out[name][:, :7], full[name][:, :7])
                else:
                    assert np.array_equal(out[name].view(np.uint8), full[name].view(np.uint8)), (want, name)


def test_max_clusters_below_the_accepted_count():
    H, W = 32, 512
    scan = M.real_scan("canyon")
    for cap in (0, 1, 17):
        models, _ = check(scan, H, W, max_clusters=cap, where=("max_clusters", cap), forms=(0,))
        assert models[0].stats[4] == 221 and models[0].stats[7] == cap and len(models[0].clusters) == cap


def test_filtered_scan_feeds_the_extraction():
    H, W = 32, 512
    c = ctx()
    for name in ("canyon", "lot"):
        scan = M.real_scan(name)
        got = c.segment_scan(scan, lidar_of(H, W))
        want = M.segment(scan, H, W)
        fe = capi.FeatureExtractionParams()
        e1, p1 = c.extract_features(got[3], lidar_of(H, W), fe)
        e2, p2 = c.extract_features(want.filtered, lidar_of(H, W), fe)
        assert len(e1) and len(p1) and np.array_equal(e1, e2) and np.array_equal(p1, p2)


def test_refusals_leave_the_outputs_untouched():
    H, W = 5, 37
    scan = M.mask_scan(M.random_mask(H, W, 4))[None]
    BAD, UNS = capi.ERR_BAD_PARAM, capi.ERR_UNSUPPORTED
    half_pi = float(np.pi / 2)
    for kw in (dict(ground_angle=float("nan")), dict(segment_angle=float("inf")), dict(ground_angle=-1e-3), dict(ground_angle=half_pi),
               dict(segment_angle=0.0), dict(segment_angle=half_pi), dict(segment_angle=-0.5)):
        run_dev(scan, H, W, capi.SegmentParams(**kw), expect=BAD)
    for max_range in (1e80, float("inf"), float("nan")):
        run_dev(scan, H, W, lidar=capi.LidarParams(H, W, 1.0, max_range), expect=BAD)
    run_dev(scan, H, W, null_scans=True, expect=BAD)
    run_dev(scan, H, W, lidar=capi.LidarParams(1, 4097, 1.0, 120.0), expect=UNS)
    run_dev(scan, H, W, lidar=capi.LidarParams(1 << 19, 2048, 1.0, 120.0), expect=UNS)  # 2^30 cells
    run_dev(scan, H, W, n_scans=65536, want=("stats",), expect=UNS)
    # null params / lidar: straight through the C ABI
    c, lib = ctx(), capi.load()
    st, lidar = capi.SegmentParams().struct(), lidar_of(H, W)
    cls = c.alloc(H * W)
    try:
        cls.upload(np.full(H * W, POISON, np.uint8))
        d = c.alloc(scan.nbytes).upload(scan)
        assert lib.loamx_segment_scans_dev(c.h, d.ptr, 1, C.byref(lidar), None, cls.ptr, None, None, None, None, 0, None) == BAD
        assert lib.loamx_segment_scans_dev(c.h, d.ptr, 1, None, C.byref(st), cls.ptr, None, None, None, None, 0, None) == BAD
        assert lib.loamx_segment_scans_dev(c.h, None, 0, C.byref(lidar), C.byref(st), cls.ptr, None, None, None, None, 0, None) == capi.OK
        c.synchronize()
        assert (cls.download(np.uint8, H * W) == POISON).all()
        d.free()
    finally:
        cls.free()
    out = (C.c_double * 2)()
    assert lib.loamx_segment_constants(None, out) == BAD and lib.loamx_segment_constants(C.byref(st), None) == BAD
    with pytest.raises(ValueError):
        c.segment_scan(np.zeros((7, 3)), lidar_of(H, W))
