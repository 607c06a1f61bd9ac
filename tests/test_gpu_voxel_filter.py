"""GPU: loamx_voxel_filter_dev — transform + voxel filter of device points — against the numpy model (map_common.py), by
equality of the count, the source indices and the output bytes. The kept set is the first point of every voxel in input
order, so nothing here depends on how the threads were scheduled."""
import functools

import numpy as np
import pytest

import map_common as M
from gpu_common import ctx
from loam_amd import capi

pytestmark = pytest.mark.gpu


def run_dev(pts, leaf, pose=None, with_idx=True, same_buffer=False):
    """loamx_voxel_filter_dev on host points -> (count, the whole n x 3 output buffer, the whole n index buffer or None)"""
    c = ctx()
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    n = len(pts)
    d_in, d_out, d_idx, d_n = c.alloc(max(pts.nbytes, 8)), c.alloc(max(pts.nbytes, 8)), c.alloc(max(4 * n, 8)), c.alloc(8)
    try:
        if n:
            d_in.upload(pts)
        d_n.upload(np.array([0xDEADBEEF, 0], dtype=np.uint32))
        c.voxel_filter_dev(d_in.ptr, n, leaf, d_in.ptr if same_buffer else d_out.ptr, d_n.ptr, d_idx.ptr if with_idx else 0, pose)
        c.synchronize()
        m = int(d_n.download(np.uint32, 1)[0])
        if n == 0:
            return m, np.empty((0, 3)), np.empty(0, dtype=np.uint32) if with_idx else None
        return m, d_out.download(np.float64, 3 * n).reshape(-1, 3), d_idx.download(np.uint32, n) if with_idx else None
    finally:
        for b in (d_in, d_out, d_idx, d_n):
            b.free()


def check(pts, leaf, want_count=None):
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    keep = M.kept_indices(pts, leaf)
    m, out, idx = run_dev(pts, leaf)
    print(f"n {len(pts)} leaf {leaf}: kept {m}, model {len(keep)}")
    assert m == len(keep)
    if want_count is not None:
        assert m == want_count
    assert np.array_equal(idx[:m], keep.astype(np.uint32))
    assert M.same_bytes(out[:m], pts[keep])
    return m


@functools.lru_cache(maxsize=None)
def room(n, seed=21):
    p = M.surface_points(np.random.default_rng(seed), n)
    p.setflags(write=False)
    return p


@pytest.mark.parametrize("leaf", [0.4, 0.2])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1025, 24_000])
def test_sizes_around_the_wavefront_and_the_tile(n, leaf):
    check(room(24_000)[:n], leaf)


def test_300k_points_take_several_rounds_of_the_tile_scan():
    # 1 172 tiles of 256 points: the one-workgroup scan of the tile counts walks them 256 at a time, so this size is past
    # the first round (65 536 points) and ends in a partial one; there is no further level for a larger n to reach
    m = check(room(300_000, seed=22), 0.1)
    assert 100_000 < m < 200_000  # (the generator's density: about half of the points survive at this leaf)


def test_the_tile_scan_at_its_round_boundary():
    for n in (256 * 256 - 1, 256 * 256, 256 * 256 + 1):
        check(room(300_000, seed=22)[:n], 0.2)


def test_one_voxel_and_all_distinct_voxels():
    rng = np.random.default_rng(23)
    one = np.array([3.2, -2.0, 1.2]) + rng.uniform(0.01, 0.39, (5000, 3))  # (inside one voxel of 0.4 m)
    assert len(np.unique(M.voxel_keys(one, 0.4)[0])) == 1
    assert check(one, 0.4) == 1  # 5 000 threads contend for one slot: point 0 wins
    g = np.stack(np.meshgrid(np.arange(20), np.arange(25), np.arange(10), indexing="ij"), -1).reshape(-1, 3)[rng.permutation(5000)]
    distinct = (g - 7 + 0.5) * 0.4  # voxel centres (an offset of half a leaf would put them on the faces)
    assert len(np.unique(M.voxel_keys(distinct, 0.4)[0])) == 5000
    assert check(distinct, 0.4) == 5000


def test_every_point_three_times():
    base = room(24_000)[:4000]
    rng = np.random.default_rng(24)
    pts = np.concatenate([base, base, base])[rng.permutation(12_000)]
    m = check(pts, 0.2)
    assert m == len(M.kept_indices(base, 0.2))


def test_lattice_of_exact_leaf_multiples():
    for leaf in (0.4, 0.2, 0.1):
        lat = np.arange(-50, 50) * leaf  # points ON voxel faces: floor(p / leaf) falls on both sides of the integers
        pts = np.stack(np.meshgrid(lat[::3], lat[::4], lat[::5], indexing="ij"), -1).reshape(-1, 3)
        pts = np.concatenate([pts, pts + leaf * 0.5, np.stack([lat, lat, lat], 1), -np.stack([lat, lat, lat], 1)])
        check(pts, leaf)


def test_non_finite_and_out_of_range_points_are_dropped():
    pts = room(24_000)[:3000].copy()
    pts[10, 0], pts[500, 1], pts[2999, 2] = np.nan, np.inf, 1e9
    pts[0] = [0.4 * M.BIAS, 0.0, 0.0]  # the range edge itself: out
    keep = M.kept_indices(pts, 0.4)
    assert not np.isin([0, 10, 500, 2999], keep).any()
    check(pts, 0.4)


def test_same_call_twice_same_bytes_and_null_src_idx():
    pts = room(24_000)
    m1, out1, idx1 = run_dev(pts, 0.2)
    m2, out2, idx2 = run_dev(pts, 0.2)
    assert m1 == m2 and M.same_bytes(out1[:m1], out2[:m2]) and np.array_equal(idx1[:m1], idx2[:m2])
    m3, out3, none = run_dev(pts, 0.2, with_idx=False)
    assert none is None and m3 == m1 and M.same_bytes(out3[:m3], out1[:m1])


def test_pose_forms(oracle):
    rng = np.random.default_rng(25)
    pts = room(24_000).copy()
    pts[5] = [-0.0, 0.0, -0.0]
    # leaf <= 0: everything is kept, in place and order; the identity (NULL, or exactly 0 0 0 1 0 0 0) returns the bits
    for leaf in (0.0, -1.0):
        for pose in (None, M.IDENTITY):
            m, out, idx = run_dev(pts, leaf, pose)
            assert m == len(pts) and M.same_bytes(out, pts) and np.array_equal(idx, np.arange(len(pts), dtype=np.uint32))
    m, out, idx = run_dev(pts, 0.4, M.IDENTITY)
    keep = M.kept_indices(pts, 0.4)
    assert m == len(keep) and M.same_bytes(out[:m], pts[keep])
    # a general pose: the arithmetic of the association's *_moved, within the bound tests/test_gpu_direct.py holds that to
    q = rng.normal(size=4)
    pose = np.concatenate([q / np.linalg.norm(q), [1.5, -2.5, 0.75]])
    m, moved, idx = run_dev(pts, 0.0, pose)
    assert m == len(pts)
    want = np.stack([oracle.pose_act(pose, p) for p in pts[:3000]])
    err = np.abs(moved[:3000] - want).max()
    print(f"pose_act: max error {err:.3e}")
    assert err <= 1e-12 * (1 + np.abs(pts).max())
    # ... and the filter with that pose is the model applied to the library's own transformed points, exactly
    keep = M.kept_indices(moved, 0.4)
    m, out, idx = run_dev(pts, 0.4, pose)
    assert m == len(keep) and np.array_equal(idx[:m], keep.astype(np.uint32)) and M.same_bytes(out[:m], moved[keep])
    # the host convenience returns the same
    hp, hi = ctx().voxel_filter(pts, 0.4, pose)
    assert M.same_bytes(hp, moved[keep]) and np.array_equal(hi, keep.astype(np.uint32))


def test_bad_parameters():
    pts = room(24_000)[:100]
    for kw in (dict(same_buffer=True), dict(leaf=float("nan")), dict(pose=[0, 0, np.nan, 1, 0, 0, 0]), dict(pose=[0, 0, 0, 1, np.inf, 0, 0])):
        with pytest.raises(capi.LoamxError) as e:
            run_dev(pts, kw.pop("leaf", 0.4), **kw)
        assert e.value.status == capi.ERR_BAD_PARAM
    m, out, idx = run_dev(pts, 0.4)  # the context works on
    assert m == len(M.kept_indices(pts, 0.4))
