"""GPU: the deal of the live pairs over the XCD lanes (ICF iterations 3+, xcd_map.h: xcd_live_map; register_kernels.hip:
live_list) places workgroups and changes no result. Batches of 8 ... 24 scan pairs (32 x 512 scans of the seeded room, the
shape of test_gpu_register's batch test) mix pairs that stop after one or two iterations — a scan against itself, the
generator's own motion — with pairs that need three, four or five — the generator's motion, the source scan turned and
shifted some more — so that 0, 1, 7, 8, 9, all but one and all pairs of a batch enter the third iteration, unevenly over the
lanes xcd_pair_map gives them. Which pair needs how many iterations was read off the CPU oracle (the GPU path reproduces its
iteration counts, test_gpu_register.py); the tests assert the counts they rely on from the records themselves.

Every batch's records equal, byte for byte: each pair registered alone (a one-pair call has no lists), the same batch under
NO_LIVE_DEAL, and the batch reversed."""
import functools

import numpy as np
import pytest

from gpu_common import ctx, option
from loam_amd import capi

pytestmark = pytest.mark.gpu

H, W, N, SEED = 32, 512, 32 * 512, 13
REC = capi.INFORMATION_DTYPE

# pair recipes and the ICF iterations each needs
SAME = [("same", p) for p in range(4)]                                              # 1
TWO = [("synth", p) for p in (1, 2, 5, 6, 7, 8, 9, 12)]                             # 2
THREE = [("synth", p) for p in (0, 3, 4, 10, 11, 15, 20, 24, 30, 32, 33)]           # 3
FOUR = [("moved", p, 0.2, (0.8, 0.4, 0.1)) for p in (0, 1, 2)]                      # 4
FIVE = [("moved", 0, 0.5, (1.5, 0.8, 0.1)), ("moved", 1, 0.4, (1.2, 0.6, 0.1))]     # 5
WANT = {**{k: 1 for k in SAME}, **{k: 2 for k in TWO}, **{k: 3 for k in THREE}, **{k: 4 for k in FOUR}, **{k: 5 for k in FIVE}}
QUICK, SLOW = SAME + TWO, THREE + FOUR + FIVE


def _place(n_pairs, slow_at, slow, quick):
    """a batch of n_pairs recipes: `slow` at the positions slow_at, `quick` everywhere else"""
    slow, quick = list(slow), list(quick)
    return [slow.pop(0) if p in slow_at else quick.pop(0) for p in range(n_pairs)]


# name -> (recipes, pairs that enter the third iteration). The slow pairs sit on few XCD lanes (position % 8) where they can.
BATCHES = {
    "8_none": (_place(8, (), [], QUICK), 0),
    "9_one": (_place(9, (4,), FOUR, QUICK), 1),
    "15_seven": (_place(15, (0, 8, 1, 9, 2, 10, 3), [THREE[0], FOUR[0], THREE[1], FIVE[0], THREE[2], FOUR[1], THREE[3]], QUICK), 7),
    "16_eight": (_place(16, (0, 1, 2, 3, 8, 9, 10, 11), THREE[4:9] + [FOUR[2], FIVE[1], FOUR[0]], QUICK), 8),
    "17_nine": (_place(17, (0, 8, 16, 1, 9, 5, 13, 6, 7), THREE[:4] + FOUR[:2] + FIVE + [THREE[9]], QUICK), 9),
    "24_all_but_one": (_place(24, set(range(24)) - {11}, THREE + FOUR + FIVE + THREE[:7], QUICK), 23),
    "16_all": (_place(16, set(range(16)), THREE[:9] + FOUR + FIVE + THREE[9:], []), 16),
}


def lidar():
    return capi.LidarParams(H, W, 1.0, 120.0)


@functools.lru_cache(maxsize=None)
def scans(recipe):
    """(target scan, source scan) of a recipe, each N x 3"""
    kind, p = recipe[0], recipe[1]
    tgt = capi.synth_scan_host(SEED, p, 0, H, W, 0.01)
    if kind == "same":
        return tgt, tgt
    src = capi.synth_scan_host(SEED, p, 1, H, W, 0.01)
    if kind == "moved":
        yaw, shift = recipe[2], recipe[3]
        c, s = np.cos(yaw), np.sin(yaw)
        src = np.ascontiguousarray(src @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]).T + np.asarray(shift))
    return tgt, src


def stacked(recipes):
    return np.ascontiguousarray(np.stack([np.stack(scans(r)) for r in recipes]))  # (P, 2, N, 3), target first


def run(recipes, want_info=False):
    """one loamx_register_scan_pairs_dev call: the records as bytes [P][64] (and the information records)"""
    c, P = ctx(), len(recipes)
    xyz = stacked(recipes)
    d_xyz, d_res, d_info = c.alloc(xyz.nbytes).upload(xyz), c.alloc(P * 64), c.alloc(P * REC.itemsize)
    try:
        c.register_scan_pairs_dev(d_xyz.ptr, P, lidar(), capi.FeatureExtractionParams(), capi.RegistrationParams(), d_res.ptr,
                                  d_info=d_info.ptr if want_info else None)
        c.synchronize()
        res = d_res.download(np.uint8, P * 64).reshape(P, 64).copy()
        return (res, d_info.download(REC, P).copy()) if want_info else res
    finally:
        d_xyz.free(), d_res.free(), d_info.free()


@functools.lru_cache(maxsize=None)
def alone(recipe):
    """the pair in a call of its own: the reference of every batch that holds it (computed once)"""
    res = run([recipe])[0]
    res.setflags(write=False)
    return res


def singles(recipes):
    return np.stack([alone(r) for r in recipes])


def iterations(res):
    return np.ascontiguousarray(res).view(capi.RESULT_DTYPE)["iterations"].ravel()


def check_mix(name, res):
    """the batch really is the mix its name says (a failure, not a skip, if the scans no longer give it)"""
    recipes, live3 = BATCHES[name]
    it = iterations(res)
    assert it.tolist() == [WANT[r] for r in recipes], (name, it.tolist())
    assert int((it >= 3).sum()) == live3, (name, it.tolist())
    if 0 < live3 < len(recipes):
        assert (it <= 2).any() and (it >= 3).any()
    assert (np.ascontiguousarray(res).view(capi.RESULT_DTYPE)["termination"] == capi.CONVERGED).all()


def test_the_batches_cover_every_live_count_and_iteration_count():
    assert [len(r) for r, _ in BATCHES.values()] == [8, 9, 15, 16, 17, 24, 16]
    assert [n for _, n in BATCHES.values()] == [0, 1, 7, 8, 9, 23, 16]
    for recipes, live3 in BATCHES.values():
        assert sum(WANT[r] >= 3 for r in recipes) == live3
    its = iterations(np.stack([alone(r) for r in WANT]))
    assert its.tolist() == list(WANT.values())  # pairs that stop after 1 and 2 iterations, pairs that need 3, 4 and 5
    # the mixed batches load the XCD lanes unevenly under xcd_pair_map: what the deal is there to even out
    for name in ("15_seven", "16_eight", "17_nine"):
        lanes = np.bincount([p % 8 for p, r in enumerate(BATCHES[name][0]) if WANT[r] >= 3], minlength=8)
        assert lanes.max() - lanes.min() >= 2, name


@pytest.mark.parametrize("name", list(BATCHES))
def test_batch_equals_its_pairs_alone_the_switch_and_the_reversed_batch(name):
    recipes, _ = BATCHES[name]
    res = run(recipes)
    check_mix(name, res)
    assert np.array_equal(res, singles(recipes)), name
    with option("NO_LIVE_DEAL"):
        assert np.array_equal(run(recipes), res), name
    assert np.array_equal(run(recipes[::-1])[::-1], res), name


def test_poisoned_scratch_changes_nothing():
    recipes, _ = BATCHES["17_nine"]
    with option("DEBUG_POISON"):
        res = run(recipes)
    check_mix("17_nine", res)
    assert np.array_equal(res, singles(recipes))


def test_a_list_of_the_call_before_is_not_used():
    # 23 of 24 pairs go on in the first call; the second and third (9 pairs, one of them slow; the workspace does not grow
    # again) must not place by what the first one left
    big, small = BATCHES["24_all_but_one"][0], BATCHES["9_one"][0]
    assert np.array_equal(run(big), singles(big))
    for _ in range(2):
        res = run(small)
        check_mix("9_one", res)
        assert np.array_equal(res, singles(small))
    assert np.array_equal(run(big), singles(big))


def test_information_at_the_results_covers_every_pair():
    # the "_info" form runs one more association pass behind the solve, over ALL pairs: the solve's last list must not count
    recipes, _ = BATCHES["17_nine"]
    res, info = run(recipes, want_info=True)
    check_mix("17_nine", res)
    assert np.array_equal(res, singles(recipes))
    with option("NO_LIVE_DEAL"):
        res0, info0 = run(recipes, want_info=True)
    assert np.array_equal(res0, res) and info.tobytes() == info0.tobytes()
    assert (info["n_plane"] > 500).all() and (info["n_edge"] > 10).all()  # (no pair was left out)


def _upload_sets(c, sets, stride):
    buf = np.zeros((len(sets), stride, 3))
    for p, s in enumerate(sets):
        buf[p, :len(s)] = s
    return c.alloc(buf.nbytes).upload(buf), c.alloc(4 * len(sets)).upload(np.array([len(s) for s in sets], dtype=np.uint32))


def test_information_batch_behind_such_a_batch():
    """loamx_registration_information_batch_dev on the feature sets of the 17 pairs at their result poses, right behind the
    registration of the batch on the same context: the same records as under NO_LIVE_DEAL."""
    c = ctx()
    recipes, _ = BATCHES["17_nine"]
    P = len(recipes)
    sets = []  # [src edge, src planar, tgt edge, tgt planar] per pair
    for r in recipes:
        tgt, src = scans(r)
        (te, tp), (se, sp) = c.extract_features(tgt, lidar()), c.extract_features(src, lidar())
        sets.append((src[se], src[sp], tgt[te], tgt[tp]))
    es = max(max(len(s[0]), len(s[2])) for s in sets)
    ps = max(max(len(s[1]), len(s[3])) for s in sets)

    def information(poses):
        d = [_upload_sets(c, [s[k] for s in sets], es if k % 2 == 0 else ps) for k in range(4)]
        d_pose, d_info = c.alloc(P * 56).upload(np.ascontiguousarray(poses, dtype=np.float64)), c.alloc(P * REC.itemsize)
        try:
            c.registration_information_batch_dev(P, d[0][0].ptr, d[0][1].ptr, d[1][0].ptr, d[1][1].ptr, d[2][0].ptr, d[2][1].ptr, d[3][0].ptr,
                                                 d[3][1].ptr, es, ps, d_pose.ptr, capi.RegistrationParams(), d_info.ptr)
            c.synchronize()
            return d_info.download(REC, P).copy()
        finally:
            for b in [x for pair in d for x in pair] + [d_pose, d_info]:
                b.free()

    res = run(recipes)
    check_mix("17_nine", res)
    poses = np.ascontiguousarray(res).view(capi.RESULT_DTYPE)["pose"].reshape(P, 7)
    info = information(poses)
    with option("NO_LIVE_DEAL"):
        run(recipes)
        info0 = information(poses)
    assert info.tobytes() == info0.tobytes()
    assert (info["n_plane"] > 500).all() and (info["n_edge"] > 10).all()
