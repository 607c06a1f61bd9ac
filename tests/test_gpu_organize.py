"""GPU: loamx_organize_clouds_dev[_f32] / loamx_organize_cloud[_f32] (include/loamx.h, "unordered clouds into scans") against
the numpy model of tests/organize_common.py, by equality of bytes: the scan, src_idx and the four counters. The model reads the
layout's own tables (loamx_scan_layout_tables) and asserts that every valid point has exactly one column and monotone line
comparisons, so whatever passes here was decided by the rule, not by a rounding that two implementations happened to share."""
import ctypes as C

import numpy as np
import pytest

import organize_common as M
import outdoor_scenes as S
from gpu_common import ctx
from loam_amd import capi

pytestmark = pytest.mark.gpu

KEEPS = (capi.ORGANIZE_KEEP_FIRST, capi.ORGANIZE_KEEP_NEAREST)


def make_layout(H, W, **kw):
    return ctx().scan_layout(capi.LidarParams(H, W, 1.0, 120.0), capi.OrganizeParams(**kw))


def model(lay, pts, rings=None):
    col, tan = lay.tables()
    p = lay.params
    return M.organize(pts, lay.scan_lines, lay.points_per_line, col, tan, p.clockwise, rings, p.ring_map, p.keep)


def same(got, want, where):
    for g, w, what in zip(got, want, ("scan", "src_idx", "stats")):
        assert g.dtype == w.dtype and g.shape == w.shape, (where, what, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.flatnonzero((M.bits(g) != M.bits(w)).reshape(len(g), -1).any(axis=1)) if what == "scan" else np.flatnonzero(g != w)
        assert not len(bad), (where, what, len(bad), bad[:5].tolist(), g[bad[:5]].tolist(), w[bad[:5]].tolist())


def check_host(lay, pts, rings=None, where=""):
    got = ctx().organize_cloud(pts, lay, rings)
    want = model(lay, pts, rings)
    same(got, want, where)
    assert int(got[2].astype(np.int64).sum()) == len(pts)
    return got


def run_dev(lay, clouds, rings=None, poison=0xA5):
    """the device entry point on poisoned outputs -> [(scan, src_idx, stats) per cloud]"""
    c = ctx()
    dt = clouds[0].dtype
    f32 = dt == np.float32
    stride = clouds[0].shape[1]
    off = np.concatenate([[0], np.cumsum([len(a) for a in clouds])]).astype(np.uint64)
    pts = np.ascontiguousarray(np.concatenate(clouds, axis=0))
    n, cells, nc = len(pts), lay.cells, len(clouds)
    bufs = dict(pts=c.alloc(max(pts.nbytes, 8)), scans=c.alloc(nc * cells * 3 * dt.itemsize), src=c.alloc(nc * cells * 4), stats=c.alloc(nc * 16))
    if rings is not None:
        bufs["rings"] = c.alloc(max(2 * n, 8))
    try:
        if n:
            bufs["pts"].upload(pts)
            if rings is not None:
                bufs["rings"].upload(np.ascontiguousarray(np.concatenate(rings), dtype=np.uint16))
        for name in ("scans", "src", "stats"):
            bufs[name].upload(np.full(bufs[name].nbytes, poison, dtype=np.uint8))
        c.organize_clouds_dev(lay, bufs["pts"].ptr, stride, off, bufs["scans"].ptr, d_rings=bufs["rings"].ptr if rings is not None else 0,
                              d_src_idx=bufs["src"].ptr, d_stats=bufs["stats"].ptr, f32=f32)
        c.synchronize()
        scans = bufs["scans"].download(dt, nc * cells * 3).reshape(nc, cells, 3)
        src = bufs["src"].download(np.uint32, nc * cells).reshape(nc, cells)
        stats = bufs["stats"].download(np.uint32, nc * 4).reshape(nc, 4)
        return [(scans[i], src[i], stats[i]) for i in range(nc)]
    finally:
        for b in bufs.values():
            b.free()


@pytest.mark.parametrize("keep", KEEPS)
def test_cloud_sizes_around_the_wavefront_and_the_workgroup_at_an_odd_width(keep):
    lay = make_layout(8, 37, keep=keep, fov_bottom=-0.4, fov_top=0.2)
    rng = np.random.default_rng([61, keep])
    try:
        for n in (0, 1, 63, 64, 65, 255, 256, 257, 1025):
            scan, src, stats = check_host(lay, M.random_cloud(rng, n), where="n = %d" % n)
            if n == 1025:
                assert stats[0] > 200 and stats[3] > 100 and stats[2] > 10  # (filled, collisions and outside all occur)
    finally:
        lay.close()


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("H,W,n", [(1, 64, 300), (2, 2, 100), (16, 128, 3000), (64, 1024, 80000)])
def test_shapes_from_one_line_to_a_full_scan(H, W, n, keep):
    lay = make_layout(H, W, keep=keep, fov_bottom=-0.4, fov_top=0.2)
    try:
        scan, src, stats = check_host(lay, M.random_cloud(np.random.default_rng([62, H, W]), n), where="%d x %d" % (H, W))
        assert stats[0] > min(H * W, n) // 4
    finally:
        lay.close()


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_batch_equals_its_clouds_one_by_one_and_two_runs_give_the_same_bytes(keep, dtype):
    """clouds of 1025, 0, 64 and 300 points in one call (the launch is sized by the first): every output entry is written (the
    buffers start poisoned, with two different patterns), and each cloud's bytes are those of a call of its own"""
    lay = make_layout(8, 37, keep=keep, fov_bottom=-0.4, fov_top=0.2)
    rng = np.random.default_rng([63, keep])
    clouds = [M.random_cloud(rng, n).astype(dtype) for n in (1025, 0, 64, 300)]
    try:
        first = run_dev(lay, clouds, poison=0xA5)
        again = run_dev(lay, clouds, poison=0x3C)
        for i, cl in enumerate(clouds):
            want = model(lay, cl)
            same(first[i], want, "batch cloud %d" % i)
            same(again[i], first[i], "second run, cloud %d" % i)
            same(run_dev(lay, [cl])[0], first[i], "alone, cloud %d" % i)
            same(ctx().organize_cloud(cl, lay), first[i], "host form, cloud %d" % i)
        assert not first[1][0].any() and (first[1][1] == capi.NO_POINT).all() and not first[1][2].any()  # the empty cloud
    finally:
        lay.close()


def test_collisions_keep_first_and_keep_nearest():
    rng = np.random.default_rng(64)
    base = M.random_cloud(rng, 1500)
    n = len(base)
    tripled = np.concatenate([base, 0.5 * base, 2.0 * base])  # (scaling by a power of two keeps every point in its cell)
    lays = {k: make_layout(16, 128, keep=k, fov_bottom=-0.4, fov_top=0.2) for k in KEEPS}
    try:
        scan, src, stats = check_host(lays[capi.ORGANIZE_KEEP_FIRST], tripled, where="first")
        filled = src != capi.NO_POINT
        assert stats[3] >= 2 * stats[0] and (src[filled] < n).all()
        scan, src, stats = check_host(lays[capi.ORGANIZE_KEEP_NEAREST], tripled, where="nearest")
        assert stats[3] >= 2 * stats[0] and ((src[filled] >= n) & (src[filled] < 2 * n)).all()
        # exact duplicates: equal r2, the lowest index
        doubled = np.concatenate([base, base])
        for k in KEEPS:
            scan, src, stats = check_host(lays[k], doubled, where="duplicates")
            assert (src[src != capi.NO_POINT] < n).all()
        # two points of one cell at the two ends of a cloud of 5 000 points: the claim across workgroups
        far = M.random_cloud(rng, 5000)
        far[-1] = far[0] / 1024.0
        col, tan = lays[0].tables()
        cell = M.classify(far[:1], col, tan)[0][0]
        assert cell < M.INVALID
        scan, src, stats = check_host(lays[capi.ORGANIZE_KEEP_FIRST], far, where="ends, first")
        assert src[cell] == 0
        scan, src, stats = check_host(lays[capi.ORGANIZE_KEEP_NEAREST], far, where="ends, nearest")
        assert src[cell] == 4999 and np.array_equal(scan[cell], far[-1])
    finally:
        for lay in lays.values():
            lay.close()


@pytest.mark.parametrize("keep", KEEPS)
def test_rings_decide_the_line(keep):
    H, W = 16, 128
    rng = np.random.default_rng([65, keep])
    pts = M.random_cloud(rng, 4000)
    pts[:200, 2] = rng.uniform(40.0, 80.0, 200)  # far above the fan
    rings = rng.integers(0, H + 3, len(pts)).astype(np.uint16)
    ring_map = np.append(rng.permutation(H), [0xFFFF]).astype(np.uint16)
    plain = make_layout(H, W, keep=keep, fov_bottom=-0.4, fov_top=0.2)
    mapped = make_layout(H, W, keep=keep, fov_bottom=-0.4, fov_top=0.2, ring_map=ring_map)
    try:
        scan, src, stats = check_host(plain, pts, np.minimum(rings, H - 1), where="identity rings")
        assert stats[2] == 0
        scan, src, stats = check_host(plain, pts, rings, where="rings beyond the lines")
        assert stats[2] == (rings >= H).sum()
        scan, src, stats = check_host(mapped, pts, rings, where="ring map")  # ring H: 0xFFFF; rings H + 1, H + 2: beyond the map
        assert stats[2] == (rings >= H).sum()
        lines = np.flatnonzero(src != capi.NO_POINT) // W
        assert np.array_equal(lines, ring_map[rings[src[src != capi.NO_POINT]]])
        # without rings the points above the fan are outside; with rings they are placed
        assert (M.classify(pts[:200], *plain.tables())[0] == M.OUTSIDE).all()
        scan, src, stats = check_host(plain, pts[:200], np.minimum(rings[:200], H - 1), where="above the fan")
        assert stats[2] == 0 and stats[0] + stats[3] == 200
        same(run_dev(plain, [pts], [rings])[0], model(plain, pts, rings), "device form with rings")
    finally:
        plain.close(), mapped.close()


@pytest.mark.parametrize("keep", KEEPS)
def test_float_clouds_are_widened_for_the_rule_and_copied_bit_for_bit(keep):
    lay = make_layout(16, 128, keep=keep, fov_bottom=-0.4, fov_top=0.2)
    rng = np.random.default_rng([66, keep])
    p32 = M.random_cloud(rng, 3000).astype(np.float32)
    p32[:4] = [[3.0, -0.0, 0.1], [-0.0, 2.0, -0.0], [0.0, 0.0, 0.0], [np.nan, 1.0, 1.0]]
    try:
        scan, src, stats = check_host(lay, p32, where="float")
        assert scan.dtype == np.float32
        wide = check_host(lay, p32.astype(np.float64), where="widened")
        assert np.array_equal(src, wide[1]) and np.array_equal(stats, wide[2])
        assert np.array_equal(M.bits(scan.astype(np.float64)), M.bits(wide[0]))
        filled = src != capi.NO_POINT
        assert np.array_equal(M.bits(scan[filled]), M.bits(p32[src[filled]]))  # the input's own bits, -0.0 included
        assert 0 in src[filled] and 1 in src[filled] and np.signbit(scan[src == 0][0, 1]) and stats[1] == 2
        # x y z intensity with garbage in the fourth scalar
        p4 = np.concatenate([p32, np.full((len(p32), 1), np.nan, dtype=np.float32)], axis=1)
        same(ctx().organize_cloud(p4, lay), (scan, src, stats), "stride 4")
        same(run_dev(lay, [p4])[0], (scan, src, stats), "stride 4, device form")
        p4d = np.concatenate([p32.astype(np.float64), np.full((len(p32), 1), np.nan)], axis=1)
        same(ctx().organize_cloud(p4d, lay), wide, "stride 4, double")
    finally:
        lay.close()


@pytest.mark.parametrize("name", S.SCENES)
def test_round_trip_of_an_outdoor_scan_through_a_shuffle(name):
    """a canyon, a lot and a field scan at 32 x 256 with their own fans: shuffled, no-return beams left in, organised again"""
    H, W = 32, 256
    c = ctx()
    origin, yaw = S.sensor_origin(name, 0)
    scan = S.scan_at(name, 0, origin, yaw, H=H, W=W)
    no_return = (scan == 0).all(axis=1)
    perm = np.random.default_rng(67).permutation(H * W)
    lidar = capi.LidarParams(H, W, 1.0, 120.0)
    feats = c.extract_features(scan, lidar)
    for keep in KEEPS:
        lay = c.scan_layout(lidar, capi.OrganizeParams(keep=keep, elevations=M.fan_elevations(H, S.FANS[name])))
        try:
            got, src, stats = check_host(lay, scan[perm], where=name)
            assert np.array_equal(got, scan)  # value-equal everywhere (an empty cell is +0, a no-return beam may hold -0) ...
            assert np.array_equal(M.bits(got[~no_return]), M.bits(scan[~no_return]))  # ... byte-equal on the filled cells
            inverse = np.empty(H * W, dtype=np.int64)
            inverse[perm] = np.arange(H * W)
            assert np.array_equal(src[~no_return], inverse[~no_return]) and (src[no_return] == capi.NO_POINT).all()
            assert stats.tolist() == [int((~no_return).sum()), int(no_return.sum()), 0, 0] and no_return.sum() > 0
            again = c.extract_features(got, lidar)
            assert np.array_equal(again[0], feats[0]) and np.array_equal(again[1], feats[1]) and len(feats[0]) and len(feats[1])
        finally:
            lay.close()


def test_clockwise_with_an_azimuth_zero():
    for keep in KEEPS:
        lay = make_layout(16, 128, keep=keep, clockwise=True, azimuth_zero=0.3, elevations=np.sort(np.random.default_rng(68).uniform(-0.5, 0.3, 16)))
        try:
            pts = M.random_cloud(np.random.default_rng(69), 5000)
            scan, src, stats = check_host(lay, pts, where="clockwise")
            filled = np.flatnonzero(src != capi.NO_POINT)
            az = np.arctan2(scan[filled, 1], scan[filled, 0])
            d = np.angle(np.exp(1j * (az - (0.3 - 2 * np.pi * (filled % 128) / 128))))
            assert np.abs(d).max() <= np.pi / 128 * (1 + 1e-9)
        finally:
            lay.close()


def test_refusals_leave_the_outputs_untouched():
    c = ctx()
    lib = c.lib
    lidar = capi.LidarParams(8, 37, 1.0, 120.0)

    def create_status(lidar, **kw):
        try:
            c.scan_layout(lidar, capi.OrganizeParams(**kw)).close()
            return capi.OK
        except capi.LoamxError as e:
            return e.status

    assert create_status(lidar) == capi.OK
    assert create_status(lidar, keep=2) == capi.ERR_BAD_PARAM
    assert create_status(lidar, azimuth_zero=np.inf) == capi.ERR_BAD_PARAM
    assert create_status(lidar, fov_bottom=0.2, fov_top=0.2) == capi.ERR_BAD_PARAM
    assert create_status(lidar, fov_bottom=np.nan) == capi.ERR_BAD_PARAM
    assert create_status(lidar, fov_bottom=-1.55, fov_top=1.55) == capi.ERR_BAD_PARAM  # the outer boundaries pass pi / 2
    assert create_status(lidar, elevations=[0, 1, 2, 3, 3, 5, 6, 7]) == capi.ERR_BAD_PARAM
    assert create_status(lidar, elevations=np.linspace(-0.3, 0.3, 8)[::-1]) == capi.ERR_BAD_PARAM
    assert create_status(lidar, ring_map=[0, 1, 8]) == capi.ERR_BAD_PARAM
    assert create_status(lidar, ring_map=[0, 1, 0xFFFF]) == capi.OK
    assert create_status(capi.LidarParams(8, 4097, 1.0, 120.0)) == capi.ERR_UNSUPPORTED
    assert create_status(capi.LidarParams(1 << 19, 4096, 1.0, 120.0)) == capi.ERR_UNSUPPORTED
    assert create_status(capi.LidarParams(0, 37, 1.0, 120.0)) == capi.ERR_BAD_PARAM
    assert create_status(capi.LidarParams(1, 37, 1.0, 120.0), fov_bottom=0.2, fov_top=0.2) == capi.OK
    with pytest.raises(ValueError):
        capi.OrganizeParams(elevations=[0.0, 0.1]).struct(8)

    lay = c.scan_layout(lidar, capi.OrganizeParams(fov_bottom=-0.4, fov_top=0.2))
    pts = M.random_cloud(np.random.default_rng(70), 100)
    cells = lay.cells
    d_pts, d_scan, d_src, d_stats = c.alloc(pts.nbytes).upload(pts), c.alloc(cells * 24), c.alloc(cells * 4), c.alloc(16)
    poison = [np.full(b.nbytes, 0x5A, dtype=np.uint8) for b in (d_scan, d_src, d_stats)]
    szp = C.POINTER(C.c_size_t)

    def call(layout, points, stride, offsets, scans):
        off = np.asarray(offsets, dtype=np.uint64)
        return lib.loamx_organize_clouds_dev(c.h, layout, points, stride, None, off.ctypes.data_as(szp), len(off) - 1, scans, d_src.ptr, d_stats.ptr)

    try:
        for b, p in zip((d_scan, d_src, d_stats), poison):
            b.upload(p)
        assert call(None, d_pts.ptr, 3, [0, 100], d_scan.ptr) == capi.ERR_BAD_PARAM
        assert call(lay.h, None, 3, [0, 100], d_scan.ptr) == capi.ERR_BAD_PARAM
        assert call(lay.h, d_pts.ptr, 2, [0, 100], d_scan.ptr) == capi.ERR_BAD_PARAM
        assert call(lay.h, d_pts.ptr, 3, [0, 60, 50], d_scan.ptr) == capi.ERR_BAD_PARAM
        assert call(lay.h, d_pts.ptr, 3, [0, 100], None) == capi.ERR_BAD_PARAM
        assert call(lay.h, d_pts.ptr, 3, [0, (1 << 32) - 1], d_scan.ptr) == capi.ERR_UNSUPPORTED
        assert lib.loamx_organize_clouds_dev(c.h, lay.h, d_pts.ptr, 3, None, None, 1, d_scan.ptr, None, None) == capi.ERR_BAD_PARAM
        assert call(lay.h, d_pts.ptr, 3, [0], d_scan.ptr) == capi.OK  # no clouds: fine, and nothing is written
        with pytest.raises(ValueError):
            c.organize_cloud(np.zeros((5, 2)), lay)
        with pytest.raises(ValueError):
            c.organize_cloud(pts, lay, rings=np.zeros(99, dtype=np.uint16))
        with pytest.raises(ValueError):
            c.organize_cloud(pts, lay, rings=np.full(100, 70000))
        with pytest.raises(ValueError):
            c.organize_clouds_dev(lay, d_pts.ptr, 3, np.array([0.0, 100.0]), d_scan.ptr)
        c.synchronize()
        for b, p in zip((d_scan, d_src, d_stats), poison):
            assert np.array_equal(b.download(np.uint8, b.nbytes), p)
        # and the accepted call works after all the refused ones
        assert call(lay.h, d_pts.ptr, 3, [0, 100], d_scan.ptr) == capi.OK
        c.synchronize()
        same((d_scan.download(np.float64, cells * 3).reshape(-1, 3), d_src.download(np.uint32, cells), d_stats.download(np.uint32, 4)),
             model(lay, pts), "after the refusals")
    finally:
        for b in (d_pts, d_scan, d_src, d_stats):
            b.free()
        lay.close()
