"""CPU-only: occupancy_math.h — ray set-up, voxel walk and voxel state of the occupancy map kernels
(loam_amd/csrc/occupancy_kernels.hip) — compiled with g++ (tests/hostcheck_occupancy) against the numpy model of
tests/occupancy_common.py, by equality. The GPU tests (test_gpu_occupancy.py) compare the kernels with the same model."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import occupancy_common as M

dp, u64p, u32p, u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)


def header_rays(pts, pose, p):
    """(kind, has_hit, outside, walks, hit_key, steps, visit lists) of the g++ build"""
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    n = len(pts)
    pose = None if pose is None else np.ascontiguousarray(pose, dtype=np.float64)
    args = (pts.ctypes.data_as(dp), C.c_uint64(n), None if pose is None else pose.ctypes.data_as(dp), C.c_double(p["leaf"]), C.c_double(p["min_range"]),
            C.c_double(p["max_range"]), C.c_double(p["end_margin"]), C.c_uint32(p["clip_long"]))
    kind, flags = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
    hit_key, steps = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
    lib = M.hostcheck_lib()
    lib.hostcheck_occupancy_rays(*args, kind.ctypes.data_as(C.POINTER(C.c_int32)), flags.ctypes.data_as(u8p), hit_key.ctypes.data_as(u64p),
                                 steps.ctypes.data_as(u32p))
    walks = (flags & 4) != 0
    lens = np.where(walks, steps.astype(np.uint64) + np.uint64(1), np.uint64(0))
    first = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    keys = np.zeros(max(int(first[-1]), 1), dtype=np.uint64)
    lib.hostcheck_occupancy_walks(*args, first.ctypes.data_as(u64p), keys.ctypes.data_as(u64p))
    lists = [keys[int(first[i]):int(first[i + 1])].tolist() for i in range(n)]
    return kind, (flags & 1) != 0, (flags & 2) != 0, walks, hit_key, steps, lists


def compare(name, p, pts, pose):
    p = dict(M.DEFAULTS, **p)
    kind, has_hit, outside, walks, hit_key, steps, lists = header_rays(pts, pose, p)
    r = M.Rays(pts, pose, p["leaf"], p["min_range"], p["max_range"], p["end_margin"], p["clip_long"])
    assert np.array_equal(kind, r.kind), name
    assert np.array_equal(has_hit, r.has_hit) and np.array_equal(outside, r.outside) and np.array_equal(walks, r.walks), name
    assert np.array_equal(hit_key, r.hit_key) and np.array_equal(steps, r.steps), name
    model_lists = r.visit_lists()
    assert lists == model_lists, name
    # the walk's invariants: sum(rem) + 1 voxels, none twice, the last one is ve's
    assert np.array_equal(r.end[r.walks], r.ve[r.walks]), name
    for i in np.flatnonzero(walks):
        assert len(lists[i]) == int(r.rem[i].sum()) + 1 == len(set(lists[i])), (name, i)
        assert lists[i][-1] == int(M.CM.pack(r.ve[i:i + 1])[0]) and lists[i][0] == int(M.CM.pack(r.v[i:i + 1])[0]), (name, i)
        hops = np.abs(np.diff(M.key_coords(lists[i]), axis=0)).sum(axis=1)
        assert (hops == 1).all(), (name, i)  # every step crosses one face
    return r


CASES = M.walk_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_model_equals_the_g_plus_plus_build_on_the_edges_of_the_rule(name):
    p, pts, pose = CASES[name]
    r = compare(name, p, pts, pose)
    if name.startswith("corner_diagonals_0.5_0.0"):
        # exact ties on two and on three axes: x goes first, then y, then z
        lists = r.visit_lists()
        d = np.diff(M.key_coords(lists[len(pts) // 3]), axis=0)
        assert d[:3].tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
        assert np.diff(M.key_coords(lists[0]), axis=0)[:2].tolist() == [[1, 0, 0], [0, 1, 0]]
    if name == "inside_one_voxel":
        assert r.walks.all() and (r.steps == 0).all()
    if name.startswith("the_end_margin_edge"):
        assert r.has_hit.all() and (~r.walks).any() and r.walks.any()
    if name.startswith("voxel_range_"):
        assert r.outside.any() or "last_voxel" in name or "plus_1" in name or "minus_1" in name
    if name in M.WALK_END_CASES:
        # long rays only: no hit anywhere, and the walk end alone decides. Exactly the ray whose ve is +-2^20 is outside and does not walk
        lost, ve = M.WALK_END_CASES[name]
        assert (r.kind == M.LONG).all() and not r.has_hit.any()
        assert r.outside.tolist() == [i == lost for i in range(3)] and r.walks.tolist() == [i != lost for i in range(3)], name
        axis = 1 if "_y_" in name else 0
        if lost is None:
            assert abs(ve) == M.BIAS - 1 and ve in r.ve[:, axis].tolist()  # the last voxel is reached ...
        else:
            assert abs(ve) == M.BIAS and (np.abs(r.ve) < M.BIAS).all()  # ... the one behind it is not (ve of a ray without a walk is 0 here)
            end = pose[4 + axis] + (1 if ve > 0 else -1) * p["max_range"]  # max_range from the origin, along the axis
            assert np.floor(end / p["leaf"]) == ve  # (the case does put the walk end in voxel +-2^20)


def test_the_model_equals_the_g_plus_plus_build_on_random_rays_at_four_leaves():
    pts, pose = M.random_rays()
    for leaf in (0.2, 0.4, 0.1, 1.0):
        compare(leaf, dict(leaf=leaf), pts, pose)
    compare("no pose", dict(leaf=0.4), pts, None)
    compare("float input", dict(leaf=0.4), pts.astype(np.float32).astype(np.float64), pose)


def test_the_state_rule_at_both_edges_of_each_threshold():
    for min_hits, ratio, min_passes in ((1, 0.0, 1), (3, 0.0, 2), (1, 0.5, 1), (2, 0.25, 5), (0, 0.0, 0), (1, 1e-9, 1), (1, 3.0, 1)):
        hs = sorted({0, 1, 2, 3, 4, 7, 8, max(min_hits - 1, 0), min_hits, min_hits + 1, (1 << 32) - 2})
        ps = sorted({0, 1, 2, 3, 4, 5, 6, 8, 15, 16, 17, 32, max(min_passes - 1, 0), min_passes, min_passes + 1, (1 << 32) - 2})
        hits, passes = [a.ravel().astype(np.uint32) for a in np.meshgrid(hs, ps)]
        out = np.zeros(len(hits), dtype=np.uint8)
        M.hostcheck_lib().hostcheck_occupancy_states(hits.ctypes.data_as(u32p), passes.ctypes.data_as(u32p), C.c_uint64(len(hits)), C.c_uint32(min_hits),
                                                     C.c_double(ratio), C.c_uint32(min_passes), out.ctypes.data_as(u8p))
        assert np.array_equal(out, M.state(hits, passes, min_hits, ratio, min_passes)), (min_hits, ratio, min_passes)
    s = lambda h, p, **kw: int(M.state([h], [p], **kw)[0])
    assert (s(0, 0), s(0, 1), s(1, 0), s(1, 1000)) == (M.UNKNOWN, M.FREE, M.OCCUPIED, M.OCCUPIED)
    assert (s(2, 5, min_hits=3), s(3, 5, min_hits=3), s(2, 0, min_hits=3)) == (M.FREE, M.OCCUPIED, M.UNKNOWN)
    assert (s(1, 2, occ_ratio=0.5), s(1, 3, occ_ratio=0.5), s(2, 4, occ_ratio=0.5), s(2, 5, occ_ratio=0.5)) == (M.OCCUPIED, M.FREE, M.OCCUPIED, M.FREE)
    assert (s(0, 1, min_passes=2), s(0, 2, min_passes=2)) == (M.UNKNOWN, M.FREE)


def test_the_model_map_counts_hits_passes_and_every_drop():
    """A check of the REFERENCE only: the numpy model against numbers worked out by hand. It runs no code of the library (and so
    passes without it); the library is covered by the comparisons with the g++ build above and by the GPU tests."""
    m = M.OccupancyModel(leaf=1.0, min_range=0.5, max_range=10.0, end_margin=0.0)
    pts = np.array([[3.5, 0.5, 0.5], [3.5, 0.5, 0.5], [0, 0, 0], [np.nan, 0, 0], [0.5, 20.0, 0.5], [2.5, 0.5, 0.5]])
    m.add(pts)
    counts, st = m.box([0, 0, 0], [5, 1, 1])
    assert counts[0, 0].tolist() == [[0, 4], [0, 3], [1, 2], [2, 0], [0, 0]] and st[0, 0].tolist() == [1, 1, 2, 2, 0]
    assert m.stats() == dict(rays_offered=6, rays_hit=3, invalid=1, range_short=1, range_long=1, outside=0, visits=8 + 10, voxels=4 + 9, overflow=0)
    assert m.slice([0, 0, 0], [5, 2, 1]).tolist() == [[1, 1, 2, 2, 0], [1, 0, 0, 0, 0]]
    c, s = m.query(np.array([[2.2, 0.1, 0.9], [0.5, 9.5, 0.5], [0.5, 10.5, 0.5], [1e9, 0, 0]]))
    assert c.tolist() == [[1, 2], [0, 1], [0, 0], [0, 0]] and s.tolist() == [2, 1, 0, 0]
    assert (m.plain_claims, m.wave_claims) == (3 + 18, 2 + 2 + 3 + 2 + 1 + 6)


def test_the_same_functions_are_clean_under_asan_and_ubsan_in_a_stand_alone_program():
    subprocess.check_call(["make", "-s", "-C", M.HOSTCHECK_DIR, "san"])
    out = subprocess.run([os.path.join(M.HOSTCHECK_DIR, "hostcheck_occupancy_san")], capture_output=True, text=True, timeout=300)
    text = out.stdout + out.stderr
    assert out.returncode == 0 and "hostcheck_occupancy ok" in out.stdout, text[-3000:]
    assert "runtime error" not in text and "AddressSanitizer" not in text, text[-3000:]
