"""Feature-set pairs that send the LM solve kernels (sweep_kernel, moment_kernel, lm_step_kernel, lm_pair_loop_kernel; DESIGN.md
4.6) through every form of their record walks. numpy only, seeded: tests/test_solve_forms_hostcheck.py asserts on the CPU that
each scene has the form it is named for, tests/test_gpu_solve_forms.py asserts the same from the library's readout
(loamx_ctx_last_solve_census) and compares the results with the oracle.

A scene: target sets on three planes and three lines of a room, the source sets an exact-size subset of them, moved and noisy;
`n_out` of the source planar points are pushed 0.6 - 1.4 m ALONG THEIR PLANE'S NORMAL: their neighbours stay within the 2 m search
radius, so they are associated, and their residual stays above kMomInlier = 0.5, so the moment pass lists them."""
import collections

import numpy as np

import reference_kats as K

# the kernels' constants (loam_amd/csrc/loamx_internal.h; both test files assert that these are the ones in use)
SWEEP_THREADS, SWEEP_CHUNK, EDGE_CACHE, LIST_CACHE, FLAT_CACHE = 256, 4096, 320, 64, 192
MOM_INLIER = 0.5

Scene = collections.namedtuple("Scene", "name se sp te tp min_assoc expect")


def n_tiles(planar_stride):
    """moment tiles per pair of a call with this plane capacity (reg_prepare: mom_blocks_per_pair * 4)"""
    return 4 * ((max(1, planar_stride) + SWEEP_CHUNK - 1) // SWEEP_CHUNK)


def live_tiles(planar_stride, n_sp):
    return min(n_tiles(planar_stride), 4 * ((n_sp + SWEEP_CHUNK - 1) // SWEEP_CHUNK))


def walk_of(planar_stride, listed):
    """the walk lm_pair_loop_kernel takes over `listed` records: 'flat', 'count' (tiled: too many records) or 'tiles' (tiled:
    the call's capacity makes more tiles than the kernel keeps counts for)"""
    return "tiles" if n_tiles(planar_stride) > LIST_CACHE else ("count" if listed > FLAT_CACHE else "flat")


def make(seed, n_se, n_sp, n_out=0, cluster=0, n_te=None, n_tp=None, centre=(0.0, 0.0, 0.0), angle=None, shift=0.03):
    """(src_edge, src_planar, tgt_edge, tgt_planar) with exactly n_se / n_sp source points. cluster: the outliers are the source
    points of ONE plane nearest to that many spots on it (neighbours in space, hence in the Morton order of the source slots)
    instead of spread over the scene. centre: where the room stands; the motion rotates about it."""
    rng = np.random.default_rng(seed)
    n_te = (n_se + n_se // 8 + 2 if n_se else 0) if n_te is None else n_te
    n_tp = n_sp + n_sp // 8 + 8 if n_tp is None else n_tp
    centre = np.asarray(centre, float)
    pts, nrm, pid = [], [], []
    for k in range(3):
        o, u, v = rng.normal(size=3) * 3, rng.normal(size=3), rng.normal(size=3)
        u, v = u / np.linalg.norm(u), v / np.linalg.norm(v)
        n = np.cross(u, v)
        pts.append(o + np.outer(rng.uniform(-4, 4, n_tp), u) + np.outer(rng.uniform(-4, 4, n_tp), v))
        nrm.append(np.tile(n / np.linalg.norm(n), (n_tp, 1)))
        pid.append(np.full(n_tp, k))
    keep = rng.permutation(3 * n_tp)[:n_tp]
    tp, tn, tpid = np.concatenate(pts)[keep], np.concatenate(nrm)[keep], np.concatenate(pid)[keep]
    te = np.zeros((0, 3))
    if n_te:
        te = np.concatenate([rng.normal(size=3) * 4 + np.outer(np.linspace(-3, 3, max(2, n_te // 3 + 1)), rng.normal(size=3)) for _ in range(3)])[:n_te]
    ax = rng.normal(size=3)
    q = K.quat_angle_axis(rng.uniform(0, 0.03) if angle is None else angle, ax / np.linalg.norm(ax))
    t = rng.normal(size=3) * shift
    T = K.pose7(q, t)
    sub_e = np.sort(rng.permutation(len(te))[:n_se])
    sub_p = np.sort(rng.permutation(n_tp)[:n_sp])
    sp0, sn = tp[sub_p].copy(), tn[sub_p]
    if n_out:
        if cluster:  # `cluster` patches of plane 0, n_out points in all
            mine = np.nonzero(tpid[sub_p] == 0)[0]
            out = np.zeros(0, dtype=np.int64)
            for k in range(int(cluster)):
                rest = np.setdiff1d(mine, out)
                spot = sp0[rest[rng.integers(len(rest))]]
                out = np.concatenate([out, rest[np.argsort(np.linalg.norm(sp0[rest] - spot, axis=1))[:(n_out * (k + 1)) // int(cluster) - len(out)]]])
        else:
            out = rng.permutation(n_sp)[:n_out]
        assert len(out) == n_out
        sp0[out] += sn[out] * (rng.uniform(0.6, 1.4, n_out) * rng.choice([-1.0, 1.0], n_out))[:, None]
    se = K.transform_points(T, te[sub_e]) + rng.normal(size=(n_se, 3)) * 0.002 if n_se else np.zeros((0, 3))
    sp = K.transform_points(T, sp0) + rng.normal(size=(n_sp, 3)) * 0.002
    c = np.ascontiguousarray
    return c(se + centre), c(sp + centre), c(te + centre), c(tp + centre)


SE_COUNTS = (0, 1, 319, 320, 321, 700)  # source edge slots on both sides of the EDGE_CACHE records kept in LDS
SP_COUNTS = (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193)  # source plane slots against the wavefront / chunk sizes

# name: (seed, n_se, n_sp, make's keywords, min_associations, what the scene is for). Expectations ("expect"):
#   walk          the walk of every iteration's listed records at the scene's own capacity ('flat' / 'count')
#   listed        (lo, hi): every iteration lists that many records (the margins to FLAT_CACHE = 192 are part of the case)
#   every_tile    every live tile lists some record
#   big_and_hole  some tile lists more than 64 records (a second trip of the tile walk) and an empty tile lies between non-empty ones
#   min_iters     the solve runs at least that many ICF iterations
#   streams       at some iteration >= 1 the accepted update is outside the moments' validity bound (left-hand side >= 2), which
#                 holds at the identity update (< 0.999): the solve switched to streaming the records in its middle
#   calm          the bound's left-hand side at the accepted update is <= 0.5 in every iteration
_FAR = dict(n_out=30, angle=0.12)
_SPECS = collections.OrderedDict([
    ("flat_none", (1, 60, 3000, {}, 100, dict(walk="flat", listed=(0, 0)))),
    ("flat_one", (2, 60, 3000, dict(n_out=1), 100, dict(walk="flat", listed=(1, 1)))),
    ("flat_140", (3, 60, 3000, dict(n_out=150), 100, dict(walk="flat", listed=(100, FLAT_CACHE - 40)))),
    ("count_spread", (4, 60, 3000, dict(n_out=400), 100, dict(walk="count", listed=(FLAT_CACHE + 40, 400), every_tile=True))),
    ("count_cluster", (32, 60, 5000, dict(n_out=260, cluster=1), 100, dict(walk="count", listed=(FLAT_CACHE + 40, 260), big_and_hole=True))),
    ("changeover", (300, 320, 3900, dict(n_out=100), 100, dict(walk="flat"))),  # n_se + n_sp crosses SWEEP_CHUNK inside the planes
    ("edge_only", (61, 700, 0, dict(angle=0.08), 50, dict(walk="flat", listed=(0, 0), min_iters=2))),
    ("plane_only", (7, 0, 9000, dict(n_out=600), 100, dict(walk="count", listed=(FLAT_CACHE + 40, 600), min_iters=2))),
    ("far_stream", (110, 60, 3000, dict(centre=(60.0, 5.0, -3.0), **_FAR), 100, dict(walk="flat", streams=True))),
    ("near_twin", (110, 60, 3000, _FAR, 100, dict(walk="flat", calm=True))),
] + [("se_%d" % n, (70 + n, n, 600, dict(n_out=20), 100, dict(walk="flat"))) for n in SE_COUNTS]
  + [("sp_%d" % n, (200 + n, 60, n, dict(n_out=n // 12), 20, {})) for n in SP_COUNTS])
# not solve forms, but what a batch must also carry: a pair that ends with too few associations, one that converges at once
_EXTRA = collections.OrderedDict([
    ("too_few", (301, 10, 40, {}, 100, {})),
    ("at_once", (302, 60, 600, dict(angle=1e-5, shift=1e-5), 100, {})),
])
NAMES = tuple(_SPECS)
EXTRA_NAMES = tuple(_EXTRA)
# the scenes that go through the "_dev" entry point at a plane capacity of more than LIST_CACHE tiles: both list sizes
TILES_NAMES = ("flat_140", "count_spread")
BIG_STRIDE = LIST_CACHE // 4 * SWEEP_CHUNK + 1  # 65 537 slots: the first capacity with more than LIST_CACHE tiles

_cache = {}


def scene(name):
    if name not in _cache:
        seed, n_se, n_sp, kw, min_assoc, expect = (_SPECS.get(name) or _EXTRA[name])
        _cache[name] = Scene(name, *make(seed, n_se, n_sp, **kw), min_assoc, expect)
    return _cache[name]
