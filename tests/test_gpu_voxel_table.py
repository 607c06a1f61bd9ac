"""GPU: what the voxel filter, the cloud map and the occupancy map share (loam_amd/csrc/voxel_table.h and the chunk walk of
api_host.h), held to the numpy models of tests/cloudmap_common.py and tests/occupancy_common.py by equality of bytes:
the cloud map over more clouds than one launch takes, and the probe of a table so small that it runs past the table's end."""
import ctypes as C

import numpy as np
import pytest

import cloudmap_common as CM
import occupancy_common as OM
import test_gpu_cloudmap as TC
import test_gpu_occupancy as TO
import test_map_hostcheck as MH
from gpu_common import ctx, option
from loam_amd import capi
from map_common import small_pose

pytestmark = pytest.mark.gpu


# ---- 1. the cloud map, more clouds than one launch --------------------------------------------------------------------------
def many_clouds():
    """600 clouds of 0 to 3 points: the offsets of 256 travel with a launch, so the call is three chunks; the clouds at both
    sides of the chunk boundaries are empty, and so are several in a row inside a chunk and at both ends of the call"""
    rng = np.random.default_rng(51)
    sizes = rng.integers(0, 4, 600)
    sizes[[0, 255, 256, 511, 599]] = 0
    sizes[100:105] = 0
    sizes[510:514] = 0
    assert sizes.max() == 3 and (sizes[257:510] > 0).any()
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    pts = rng.uniform(-1.5, 1.5, (int(offsets[-1]), 3)) * [1.0, 1.0, 0.2]
    poses = np.stack([small_pose(rng, angle=0.3, shift=1.0) for _ in sizes])
    return pts, offsets, poses


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_cloud_map_takes_more_clouds_than_one_launch_with_their_own_poses(dtype):
    xyz, offsets, poses = many_clouds()
    pts = xyz.astype(dtype)
    c = ctx()
    model = CM.CloudMapModel(0.5, 0.5, 120.0)
    model.add(pts, offsets, poses)
    whole = []
    for plain in (0, 1):  # one call
        m, _ = TC.make()
        try:
            with option("NO_CLOUDMAP_COMBINE", plain):
                TC.dev_add(m, pts, offsets, poses)
            whole.append(TC.check(m, model, ("one call", plain)) + (m.stats().tobytes(),))
        finally:
            m.close()
    m, _ = TC.make()  # 600 calls of one cloud each, on the same device arrays
    d_pts, d_poses = c.alloc(pts.nbytes).upload(pts), c.alloc(poses.nbytes).upload(poses)
    try:
        for k in range(600):
            m.add_clouds_dev(d_pts.ptr, 3, offsets[k:k + 2], d_poses.ptr + 56 * k, f32=dtype == np.float32)
        c.synchronize()
        single = TC.check(m, model, "one cloud per call") + (m.stats().tobytes(),)
    finally:
        m.close(), d_pts.free(), d_poses.free()
    assert single[3] > 150 and single[1].max() > 2  # (shared voxels and plenty of them)
    for got in whole:
        CM.assert_emit_equal(got[:4], single[:4])
        assert got[4] == single[4]


# ---- 2. probes that run past the end of the smallest table ------------------------------------------------------------------
MAX_VOXELS, SLOTS = 8, 16  # a table has 2^k >= 2 max_voxels slots, 16 at the least
Z = 3


def numpy_hash(keys, log2_cap):
    return ((np.asarray(keys, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(64 - log2_cap)).astype(np.uint32)  # (uint64 arithmetic wraps)


def header_hash(key, log2_cap):
    """voxel_hash of map_math.h as g++ compiles it (tests/hostcheck_map)"""
    k, mx, acc = np.array([key], dtype=np.uint64), C.c_uint32(0), C.c_uint32(0)
    MH.lib().hostcheck_map_hash_range(k.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_uint64(1), C.c_uint32(log2_cap), C.byref(mx), C.byref(acc))
    return mx.value


def chosen_voxels():
    """(six voxels whose keys hash to slots 14, 15, 14, 15, 14, 15 of a table of 16, twelve other voxels); leaf 1"""
    ij = np.stack(np.meshgrid(np.arange(40), np.arange(40), indexing="ij"), -1).reshape(-1, 2)
    v = np.concatenate([ij, np.full((len(ij), 1), Z)], axis=1).astype(np.int64)
    h = numpy_hash(CM.pack(v), 4)
    at14, at15 = np.flatnonzero(h == 14), np.flatnonzero(h == 15)
    six = np.stack([at14[:3], at15[:3]], axis=1).reshape(-1)
    rest = np.setdiff1d(np.arange(len(v)), six)[:12]
    for i in np.concatenate([six, rest]):
        assert header_hash(int(CM.pack(v[i:i + 1])[0]), 4) == h[i]
    assert sorted(h[six].tolist()) == [14, 14, 14, 15, 15, 15]
    return v[six], v[rest]


SIX_ORDER = [0, 0, 1, 0, 2, 2, 2, 3, 4, 4, 5, 3, 1, 5, 5, 0]  # runs of one, two and three lanes, voxels that come back


@pytest.mark.parametrize("plain", [0, 1])
def test_cloud_map_probes_wrap_around_the_end_of_the_smallest_table(plain):
    """Six voxels for slots 14 and 15 of 16: four of them find their slot past the table's end. Twelve more voxels of one point
    each make 18 for 16 slots: the probes of two give up (a probe gives up only when every slot holds another key, and slots are
    never freed), and of the ten new voxels of the table two fit the list of 8: overflow = 2 + 8, used = all but the two."""
    six, more = chosen_voxels()
    rng = np.random.default_rng(52)
    pts6 = six[SIX_ORDER] + rng.uniform(0.1, 0.9, (len(SIX_ORDER), 3))
    pts12 = more + rng.uniform(0.1, 0.9, (12, 3))
    m = ctx().cloud_map(capi.CloudMapParams(1.0, 0.1, 120.0), MAX_VOXELS)
    model = CM.CloudMapModel(1.0, 0.1, 120.0)
    try:
        with option("NO_CLOUDMAP_COMBINE", plain):
            TC.dev_add(m, pts6)
            model.add(pts6)
            got = TC.check(m, model, "six voxels")  # centroids, counts, first (the list's order), stats
            assert got[3] == 6 and got[1].tolist() == [SIX_ORDER.count(k) for k in range(6)]
            ok, v, _ = CM.cells(pts6, 1.0)
            assert m.claims() == (len(pts6) if plain else CM.wave_runs(ok, CM.pack(v)))
            TC.dev_add(m, pts12)
            want = dict(model.stats(), voxels=MAX_VOXELS, points_offered=len(pts6) + 12, points_used=len(pts6) + 12 - (18 - SLOTS),
                        overflow=(18 - SLOTS) + (SLOTS - MAX_VOXELS))
            CM.assert_stats_equal(m.stats(), want, "eighteen voxels")
            full = TC.dev_emit(m)
            assert full[3] == MAX_VOXELS
            CM.assert_emit_equal(tuple(a[:6] for a in full[:3]) + (6,), got, "the six are as they were")
            assert (full[1][6:] == 1).all() and len(pts6) <= full[2][6] < full[2][7] < len(pts6) + 12
            m.clear()
            model.clear()
            TC.dev_add(m, pts6[::-1])
            model.add(pts6[::-1])
            TC.check(m, model, "after clear")
    finally:
        m.close()


@pytest.mark.parametrize("plain", [0, 1])
def test_occupancy_map_probes_wrap_around_the_end_of_the_smallest_table(plain):
    """The same voxels. A ray whose sensor stands in the voxel of its return visits that voxel alone, as a hit: one cloud per
    stretch of rays of a voxel, its pose a translation into the voxel. The twelve other voxels take two rays each, so the two
    voxels whose probes give up leave an overflow of four (one claim of two with combining, two claims without)."""
    six, more = chosen_voxels()
    rng = np.random.default_rng(53)
    params = dict(leaf=1.0, min_range=0.01, end_margin=0.0)

    def rays(voxels):
        """one cloud per entry: (points, offsets, poses)"""
        pts = rng.uniform(0.05, 0.3, (len(voxels), 3))
        poses = np.concatenate([np.tile([0.0, 0.0, 0.0, 1.0], (len(voxels), 1)), voxels + 0.5], axis=1)
        return pts, np.arange(len(voxels) + 1), poses

    first, second = rays(six[SIX_ORDER]), rays(np.repeat(more, 2, axis=0))
    m, model = TO.make(MAX_VOXELS, **params)
    try:
        with option("NO_OCCUPANCY_COMBINE", plain):
            TO.dev_add(m, *first)
            model.add(*first)
            TO.check(m, model, "six voxels")
            assert model.stats()["voxels"] == 6 and model.stats()["visits"] == 0
            assert m.claims() == (model.plain_claims if plain else model.wave_claims)
            counts, _ = TO.dev_query(m, six + 0.5)
            assert counts[:, 0].tolist() == [SIX_ORDER.count(k) for k in range(6)] and not counts[:, 1].any()
            TO.dev_add(m, *second)
            model.add(*second)
            want = dict(model.stats(), voxels=SLOTS, overflow=2 * (18 - SLOTS))
            OM.assert_stats_equal(m.stats(), want, "eighteen voxels")
            counts, _ = TO.dev_query(m, np.concatenate([six, more]) + 0.5)
            assert counts[:6, 0].tolist() == [SIX_ORDER.count(k) for k in range(6)] and not counts[:, 1].any()
            assert sorted(counts[6:, 0].tolist()) == [0] * (18 - SLOTS) + [2] * (SLOTS - 6)
            m.clear()
            model.clear()
            TO.dev_add(m, *first)
            model.add(*first)
            TO.check(m, model, "after clear")
            assert m.claims() == (model.plain_claims if plain else model.wave_claims)
    finally:
        m.close()
