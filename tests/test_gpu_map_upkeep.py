"""GPU: upkeep of a map held in a persistent target index — loamx_target_index_insert_filtered, _crop and _points — against a
Python model (map_common.MapModel: the point array of each kind and its occupied voxel keys) and against a fresh index built
over the model's points. Transformed points come from the library's own leaf <= 0 form, so every comparison is by equality."""
import numpy as np
import pytest

import map_common as M
from gpu_common import ctx
from loam_amd import capi

pytestmark = pytest.mark.gpu


def moved(c, pts, pose):
    """pose.act(points) as the library computes it (the leaf <= 0 form of the filter)"""
    out, idx = c.voxel_filter(pts, 0.0, pose)
    assert len(out) == len(pts)
    return out


def check_points(c, idx, model_e, model_p):
    assert c.target_index_size(idx) == (len(model_e.pts), len(model_p.pts))
    assert M.same_bytes(c.target_index_points(idx, 0), model_e.pts)
    assert M.same_bytes(c.target_index_points(idx, 1), model_p.pts)


def check_knn(c, idx, fresh, rng, model_e, model_p, n_q=300):
    for w, pts in ((0, model_e.pts), (1, model_p.pts)):
        if len(pts) == 0:
            q = rng.uniform(-5, 5, (20, 3))
            assert all(len(r) == 0 for r in c.knn_search(idx, w, q, 5, 2.0))
            continue
        q = pts[rng.integers(0, len(pts), n_q)] + rng.normal(size=(n_q, 3)) * 0.02
        for k, radius in ((5, 2.0), (8, -1.0)):
            got, ref = c.knn_search(idx, w, q, k, radius), c.knn_search(fresh, w, q, k, radius)
            assert all(np.array_equal(a, b) for a, b in zip(got, ref)), (w, k, radius)


def filtered(c, idx, me, mp, e, p, pose, le, lp):
    """one filtered insert into index and model; returns the counts (asserted equal)"""
    want = (me.insert_filtered(moved(c, e, pose), le), mp.insert_filtered(moved(c, p, pose), lp))
    got = c.target_index_insert_filtered(idx, e, p, pose, edge_leaf=le, planar_leaf=lp)
    print(f"filtered insert of {len(e)} + {len(p)} at leaves {le} / {lp}: added {got}")
    assert got == want
    check_points(c, idx, me, mp)
    return got


def test_scan_sized_map_grows_by_filtered_inserts():
    rng = np.random.default_rng(31)
    c = ctx()
    me, mp = M.MapModel(M.surface_points(rng, 900)), M.MapModel(M.surface_points(rng, 30_000))  # plain create: many points per voxel
    idx = c.target_index(me.pts, mp.pts)
    check_points(c, idx, me, mp)
    scans = []
    for i in range(4):
        e, p, pose = M.surface_points(rng, 300), M.surface_points(rng, 20_000), M.small_pose(rng)
        scans.append((e, p, pose))
        ne, npl = filtered(c, idx, me, mp, e, p, pose, 0.2, 0.4)
        assert 0 < ne < 300 and 0 < npl < 20_000  # (neither everything nor nothing: the filter has work)
    stats = c.target_index_stats(idx)
    assert filtered(c, idx, me, mp, *scans[2], 0.2, 0.4) == (0, 0)  # the same scan again adds nothing ...
    assert c.target_index_stats(idx) == stats  # ... and touches nothing
    pe, pp = M.surface_points(rng, 100), M.surface_points(rng, 5000)  # a plain insert in between: the tables catch up
    c.target_index_insert(idx, pe, pp)
    me.insert(pe), mp.insert(pp)
    check_points(c, idx, me, mp)
    assert filtered(c, idx, me, mp, pe, pp, None, 0.2, 0.4) == (0, 0)  # (its points occupy their voxels now)
    filtered(c, idx, me, mp, M.surface_points(rng, 300), M.surface_points(rng, 20_000), M.small_pose(rng), 0.2, 0.4)
    ne, npl = filtered(c, idx, me, mp, M.surface_points(rng, 300), M.surface_points(rng, 20_000), M.small_pose(rng), 0.2, 0.25)  # another leaf: table rebuilt
    assert npl > 0
    e, p = M.surface_points(rng, 300), M.surface_points(rng, 2000)
    assert filtered(c, idx, me, mp, e, p, M.small_pose(rng), 0.2, 0.0)[1] == 2000  # planar_leaf <= 0: unfiltered
    assert filtered(c, idx, me, mp, e, p, M.small_pose(rng), -1.0, 0.4)[0] == 300
    # edge-only and planar-only calls; no output pointers through the raw ABI
    filtered(c, idx, me, mp, M.surface_points(rng, 200), np.zeros((0, 3)), M.small_pose(rng), 0.2, 0.4)
    filtered(c, idx, me, mp, np.zeros((0, 3)), M.surface_points(rng, 3000), M.small_pose(rng), 0.2, 0.4)
    # the grown index against a fresh one over the model
    fresh = c.target_index(me.pts, mp.pts)
    check_knn(c, idx, fresh, rng, me, mp)
    ang = 0.01
    R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    src_p = mp.pts[rng.choice(len(mp.pts), 15_000, replace=False)] @ R.T + np.array([0.05, -0.03, 0.02])
    src_e = me.pts[rng.choice(len(me.pts), 500, replace=False)] @ R.T + np.array([0.05, -0.03, 0.02])
    a, b = c.register_features_indexed(idx, src_e, src_p), c.register_features_indexed(fresh, src_e, src_p)
    assert a[1:] == b[1:] and np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))
    c.target_index_destroy(idx)
    c.target_index_destroy(fresh)


def test_map_sized_kind_takes_filtered_inserts_by_merges():
    rng = np.random.default_rng(32)
    c = ctx()
    base_p = M.surface_points(rng, 260_000)
    base_p[:2] = [M.BOX_LO - 0.05, M.BOX_HI + 0.05]  # the grid's corners: later points stay inside (merges, not rebuilds)
    me, mp = M.MapModel(M.surface_points(rng, 900)), M.MapModel(base_p)
    idx = c.target_index(me.pts, mp.pts)
    for i in range(3):
        # a leaf at which the dense base leaves room: a few thousand new voxels per call
        ne, npl = filtered(c, idx, me, mp, M.surface_points(rng, 100), M.surface_points(rng, 30_000), None if i == 0 else M.small_pose(rng, 0.001, 0.01), 0.2, 0.1)
        assert 0 < npl < 30_000
    builds, merges = c.target_index_stats(idx)
    print(f"full builds {builds}, merges {merges}")
    assert merges >= 1
    fresh = c.target_index(me.pts, mp.pts)
    check_knn(c, idx, fresh, rng, me, mp)
    c.target_index_destroy(idx)
    c.target_index_destroy(fresh)


def test_crop():
    rng = np.random.default_rng(33)
    c = ctx()
    me, mp = M.MapModel(M.surface_points(rng, 900)), M.MapModel(M.surface_points(rng, 30_000))
    idx = c.target_index(me.pts, mp.pts)
    filtered(c, idx, me, mp, M.surface_points(rng, 300), M.surface_points(rng, 20_000), M.small_pose(rng), 0.2, 0.4)
    stats = c.target_index_stats(idx)
    big = np.array([100.0, 100.0, 100.0])
    assert c.target_index_crop(idx, -big, big) == (0, 0) and c.target_index_stats(idx) == stats  # removes nothing: nothing happens
    assert c.target_index_crop(idx, [-np.inf] * 3, [np.inf] * 3) == (0, 0) and c.target_index_stats(idx) == stats
    lo, hi = np.array([0.0, -np.inf, -50.0]), np.array([50.0, np.inf, 50.0])  # half of the room
    want = (me.crop(lo, hi), mp.crop(lo, hi))
    assert c.target_index_crop(idx, lo, hi) == want and min(want) > 0 and len(me.pts) > 0
    assert c.target_index_stats(idx) == (stats[0] + 2, stats[1])
    check_points(c, idx, me, mp)
    fresh = c.target_index(me.pts, mp.pts)
    check_knn(c, idx, fresh, rng, me, mp)
    c.target_index_destroy(fresh)
    # a filtered insert after the crop (the tables are built again: the indices have shifted); the cropped half fills again
    ne, npl = filtered(c, idx, me, mp, M.surface_points(rng, 300), M.surface_points(rng, 20_000), M.small_pose(rng), 0.2, 0.4)
    assert npl > 1000
    # a crop that empties the edge kind: the box lies to the right of every edge point
    lo3, hi3 = np.array([-np.inf, -np.inf, -np.inf]), np.array([np.inf, np.inf, np.inf])
    lo3[0] = float(me.pts[:, 0].max()) + 1e-9
    want = (me.crop(lo3, hi3), mp.crop(lo3, hi3))
    assert c.target_index_crop(idx, lo3, hi3) == want and len(me.pts) == 0
    check_points(c, idx, me, mp)
    assert c.target_index_size(idx)[0] == 0
    fresh = c.target_index(me.pts, mp.pts)
    check_knn(c, idx, fresh, rng, me, mp, n_q=50)
    c.target_index_destroy(fresh)
    # ... and the emptied kind takes points again
    filtered(c, idx, me, mp, M.surface_points(rng, 300), M.surface_points(rng, 2000), None, 0.2, 0.4)
    fresh = c.target_index(me.pts, mp.pts)
    check_knn(c, idx, fresh, rng, me, mp, n_q=50)
    c.target_index_destroy(fresh)
    c.target_index_destroy(idx)


def test_refusals_leave_the_index_as_it_was():
    rng = np.random.default_rng(34)
    c = ctx()
    me, mp = M.MapModel(M.surface_points(rng, 900)), M.MapModel(M.surface_points(rng, 30_000))
    idx = c.target_index(me.pts, mp.pts)
    filtered(c, idx, me, mp, M.surface_points(rng, 300), M.surface_points(rng, 5000), M.small_pose(rng), 0.2, 0.4)
    stats = c.target_index_stats(idx)
    e, p = M.surface_points(rng, 300), M.surface_points(rng, 5000)

    def refused(status, fn):
        with pytest.raises(capi.LoamxError) as err:
            fn()
        assert err.value.status == status, err.value
        check_points(c, idx, me, mp)
        assert c.target_index_stats(idx) == stats

    bad_p = p.copy()
    bad_p[4000, 1] = np.nan
    refused(capi.ERR_BAD_PARAM, lambda: c.target_index_insert_filtered(idx, e, bad_p, None, 0.2, 0.4))
    bad_e = e.copy()
    bad_e[7, 2] = np.inf
    refused(capi.ERR_BAD_PARAM, lambda: c.target_index_insert_filtered(idx, bad_e, p, None, 0.2, 0.4))
    refused(capi.ERR_BAD_PARAM, lambda: c.target_index_insert_filtered(idx, e, p, [0, 0, 0, 1, np.nan, 0, 0], 0.2, 0.4))
    refused(capi.ERR_BAD_PARAM, lambda: c.target_index_insert_filtered(idx, e, p, None, float("nan"), 0.4))
    far_p = p.copy()
    far_p[123] = [0.4 * M.BIAS + 1.0, 0.0, 0.0]  # finite, but floor(p / leaf) does not fit 21 bits
    refused(capi.ERR_UNSUPPORTED, lambda: c.target_index_insert_filtered(idx, e, far_p, None, 0.2, 0.4))
    refused(capi.ERR_UNSUPPORTED, lambda: c.target_index_insert_filtered(idx, e, p, [0, 0, 0, 1, 1e7, 0, 0], 0.2, 0.4))
    refused(capi.ERR_BAD_PARAM, lambda: c.target_index_crop(idx, [1.0, 0, 0], [0.0, 1, 1]))
    refused(capi.ERR_BAD_PARAM, lambda: c.target_index_crop(idx, [np.nan, 0, 0], [1.0, 1, 1]))
    refused(capi.ERR_BAD_PARAM, lambda: c.target_index_points(idx, 1, len(mp.pts) - 1, 2))
    refused(capi.ERR_BAD_PARAM, lambda: c.target_index_points(idx, 0, len(me.pts) + 1, 0))
    refused(capi.ERR_BAD_PARAM, lambda: c.target_index_points(idx, 2, 0, 1))
    assert c.target_index_points(idx, 1, len(mp.pts), 0).shape == (0, 3)  # count == 0 at the end: fine
    assert M.same_bytes(c.target_index_points(idx, 1, 100, 50), mp.pts[100:150])
    # after all that the same call, valid this time, still equals the model (the out-of-range refusals left claims in the
    # tables, which are therefore built again)
    filtered(c, idx, me, mp, e, p, M.small_pose(rng), 0.2, 0.4)
    fresh = c.target_index(me.pts, mp.pts)
    check_knn(c, idx, fresh, rng, me, mp, n_q=100)
    c.target_index_destroy(fresh)
    c.target_index_destroy(idx)
