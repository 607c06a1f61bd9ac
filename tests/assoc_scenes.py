"""Scenes for the routes of the association's k-NN queue chain, the smallest that still reach each route, with the
arithmetic that says why. Shared by tests/test_assoc_routes_hostcheck.py (CPU: the g++ build of the kernels' functions says
how many queries take each route, so a scene cannot go vacuous unseen) and tests/test_gpu_assoc_routes.py (GPU: the census of
loamx_associate must EQUAL those numbers, the lists and fits the oracle's).

Every scene is a function returning a Scene: source / target sets of both kinds, the pose (always the identity: the moved
query IS the source point, so the g++ build sees the kernels' query bit for bit) and the parameters that differ from the
defaults (k = 5, r = 2.0 planar / 1.0 edge). `kind` names the feature kind the scene is about.

grid_choose (reg_math.h): h = min(r / 4, sqrt(8 * area / n)) over the bounding box, at least r / 1000, grown by 1.1 until
nx * ny * nz <= min(65 536, max(16 n, 4096)); the grid's origin is the box's minimum."""
import collections

import numpy as np

IDENT = np.array([0, 0, 0, 1.0, 0, 0, 0])
NONE = np.zeros((0, 3))
Scene = collections.namedtuple("Scene", "name kind src_e src_p tgt_e tgt_p k_e k_p r_e r_p ties")

K_BRUTE_MAX, K_LEAN_MAX, K_COOP_MAX_SHELL, REST_THREADS = 512, 65535, 64, 64
PLAIN, WIDE, TIED = 1, 2, 3  # hostcheck_lib.knn_routes()["r1"]
REASON_WIDE, REASON_TIED = 0x80000000, 0x40000000  # capi.ASSOC_REASON_*


def scene(name, kind, src_e=NONE, src_p=NONE, tgt_e=NONE, tgt_p=NONE, k_e=5, k_p=5, r_e=1.0, r_p=2.0, ties=False):
    c = np.ascontiguousarray
    return Scene(name, kind, c(src_e, dtype=np.float64), c(src_p, dtype=np.float64), c(tgt_e, dtype=np.float64), c(tgt_p, dtype=np.float64),
                 int(k_e), int(k_p), float(r_e), float(r_p), bool(ties))


def sets(s):
    """(queries, targets, k, r) of the kind the scene is about"""
    return (s.src_p, s.tgt_p, s.k_p, s.r_p) if s.kind == "plane" else (s.src_e, s.tgt_e, s.k_e, s.r_e)


def km_of(k):
    return 5 if k <= 5 else (8 if k <= 8 else 16)


def edge_pair(rng):
    """three lines of 30 points in general position and queries a millimetre off every second point: a small edge pair
    (90 <= kBruteMax target points: brute force), which with a grid-searched planar set and k <= 5 makes the mixed launch"""
    t = np.linspace(0.0, 1.5, 30)[:, None]
    tgt = np.concatenate([np.array([2.0, -1.0, 1.5]) + t * np.array([1.0, 0.1, 0.0]), np.array([3.2, -1.0, 0.4]) + t * np.array([0.0, 1.0, 0.2]),
                          np.array([1.8, 0.2, 0.5]) + t * np.array([0.1, 0.0, 1.0])])
    return tgt[::2] + rng.normal(size=(len(tgt[::2]), 3)) * 1e-3, tgt


def wall_points(rng, n, width=8.0, height=3.0):
    """n points on the plane y = 5 with 3 mm of noise, 83 per square metre at the default size: h = sqrt(8 * 2 * 24 / 2000) =
    0.44 (below r / 4 = 0.5), one cell deep, ~16 points per cell: the 3x3 cells around a query hold ~150, its fifth neighbour is
    ~0.14 m away and the block's faces at least 0.44: round 1 finishes every query"""
    return np.column_stack([rng.uniform(-width / 2, width / 2, n), 5.0 + rng.normal(size=n) * 0.003, rng.uniform(-1.0, height - 1.0, n)])


def wall(mixed=True):
    rng = np.random.default_rng(101)
    tgt = wall_points(rng, 2000)
    src = tgt[::3] + rng.normal(size=(len(tgt[::3]), 3)) * 0.01
    se, te = edge_pair(rng) if mixed else (NONE, NONE)
    return scene("wall", "plane", se, src, te, tgt)


def sparse_points(rng, n_tgt=3000, n_src=1200, half=15.0):
    """uniform points in a 30 m cube: 0.11 per cubic metre. h = 0.5 grown to 0.886 (34^3 = 39 304 <= 16 n cells): a 3x3x3 block holds
    ~2 points, so round 1 queues (nearly) every query on its guard; the 5x5x5 block holds ~10, of which k lie inside the guard
    for about a third of the queries: the lean search finishes those and lists the rest; the radius closes at shell
    ceil(2.0 / 0.886) + 1 = 4 (+ 1 for a query outside the box)"""
    return rng.uniform(-half, half, (n_src, 3)), rng.uniform(-half, half, (n_tgt, 3))


def sparse(k=5, r=2.0, mixed=False):
    rng = np.random.default_rng(102)
    src, tgt = sparse_points(rng)
    if r <= 0:  # (no radius: h = sqrt(8 * 5400 / 3000) = 3.8, 8^3 cells; queries out to 37.5 m, most of them cells off the grid: queued)
        src = src * 2.5
    se, te = edge_pair(rng) if mixed else (NONE, NONE)
    return scene("sparse" if r > 0 else "no_radius", "plane", se, src, te, tgt, k_p=k, r_p=r)


def sparse_few():
    """the wall inside a 12 m cube of 300 uniform points (0.17 per cubic metre), 667 wall queries and 60 uniform ones: n = 2 300,
    h = r / 4 = 0.5 (24^3 cells). Only the uniform queries are queued: 60 * 4 <= rest_blocks * 64 (rest_blocks = 12: one pass over
    a full queue of 3 workgroups' worth of queries), so the rest kernel deals them out across all its workgroups"""
    rng = np.random.default_rng(103)
    w = wall_points(rng, 2000)
    tgt = np.concatenate([w, rng.uniform(-6, 6, (300, 3)) + np.array([0.0, 5.0, 0.5])])
    src = np.concatenate([w[::3] + rng.normal(size=(len(w[::3]), 3)) * 0.01, rng.uniform(-6, 6, (60, 3)) + np.array([0.0, 5.0, 0.5])])
    return scene("sparse_few", "plane", NONE, src, NONE, tgt)


def meet():
    """the target of sparse_few (2 300 points) and 2 400 queries, every one of which, in the mixed launch under FORCE_LATE_VERIFY,
    is either queued and LISTED by the two-stage chain (uniform queries the lean search does not finish) or LATE (wall queries:
    round 1 selects, the fit refuses every selection): candidates the g++ build sends any other way — finished by the rest
    kernel, or handed over with a verified count — are dropped. listed + late == n_src == the slot stride (n_src > n_tgt): the
    leftover list grows from the front of K.exact and the late list from its end, and here they meet with no slot to spare,
    filled by two streams"""
    import hostcheck_lib as Hc
    rng = np.random.default_rng(110)
    few = sparse_few()
    w = few.tgt_p[:2000]
    cand = np.concatenate([w + rng.normal(size=w.shape) * 0.01, rng.uniform(-6, 6, (1500, 3)) + np.array([0.0, 5.0, 0.5])])
    R = Hc.knn_routes(few.tgt_p, cand, 5, 2.0, True)
    keep = ((R["r1"] == 0) & R["unverified"]) | ((R["r1"] == PLAIN) & (R["lean2"] < 0))
    se, te = edge_pair(rng)
    return scene("meet", "plane", se, cand[keep][:2400], te, few.tgt_p)


def grid_of(tgt, r):
    """(origin, h, dims) of the target grid, from the g++ build of grid_choose"""
    import hostcheck_lib as Hc
    R = Hc.knn_routes(tgt, NONE, 5, r)
    return R["origin"], R["h"], np.array(R["dims"])


def cell_out(q, origin, h, dims):
    """a query's distance from the grid in cells (grid_outside_distance), in numpy: the scenes keep queries 1e-6 h off cell faces"""
    c = np.floor((np.atleast_2d(q) - origin) * (1.0 / h)).astype(np.int64)
    return np.maximum(np.maximum(-c, c - (np.asarray(dims) - 1)), 0).max(axis=1)


def outside(k=5):
    """20 000 uniform points in a 10 m cube (h = sqrt(8 * 600 / 20 000) = 0.49, 21^3 cells, ~2.4 points per cell), and queries
    `out` = 0, 1, 2, 3, 4, 5, 9 cells off the grid along each axis, on both sides, and along a diagonal, 0.37 h into their cell.
    out <= 1: round 1 searches; out = 2 .. 4: queued plain, and the cooperative search starts with out > 0;
    (out - 1) h >= r = 2.0, that is out >= 6 here (5 * 0.49 = 2.45; 4 * 0.49 = 1.96 < 2: out = 5 is still queued): count 0, not queued"""
    rng = np.random.default_rng(104)
    tgt = rng.uniform(0.0, 10.0, (20000, 3))
    origin, h, dims = grid_of(tgt, 2.0)
    qs = []
    for out in (0, 1, 2, 3, 4, 5, 9):
        for axis in range(3):
            for side in (-1, 1):
                for rep in range(4):
                    cell = rng.integers(2, dims - 2).astype(np.float64)
                    cell[axis] = -out if side < 0 else dims[axis] - 1 + out
                    qs.append(origin + (cell + 0.37) * h)
        for rep in range(4):
            qs.append(origin + (np.array([-out, dims[1] - 1 + out, -out], dtype=np.float64) + 0.37) * h)
    return scene("outside", "plane", NONE, np.array(qs), NONE, tgt, k_p=k)


def trip_budget(n):
    """n points in a cube of 0.1 m, 300 more in another far away (the set stays above kBruteMax) and three outliers that make the
    box 100 m wide: 16 n < 65 536 cells cap the table at 16^3 or fewer, h > 6 m, so each cluster lies in one cell and a query
    inside the first walks ceil(n / 4) batches on ONE row against the 64-trip budget of the pipelined walk"""
    rng = np.random.default_rng(105)
    a = rng.uniform(-0.05, 0.05, (n, 3)) + np.array([3.0, -2.0, 1.0])
    b = rng.uniform(-0.05, 0.05, (300, 3)) + np.array([-30.0, 28.0, -25.0])
    tgt = np.concatenate([a, b, [[50.0, 50, 50], [-50, -50, -50], [50, -50, 0]]])
    src = a[rng.choice(n, 40, replace=False)] + rng.normal(size=(40, 3)) * 0.003
    return scene("trip_budget_%d" % n, "plane", NONE, src, NONE, tgt)


def lattice(k, exact=True):
    """a 9 x 9 x 8 lattice at 0.125 m from (2, -1, 0.5) — every coordinate, every offset from the grid origin and every squared
    distance is exact in FP32 and FP64 alike — and 300 of its points as queries: the nearest is the point itself, the next
    six are EXACTLY equidistant. k = 5 (mixed launch): the round-1 selection cannot be verified, the fit refuses it: late list.
    k = 6 (KM = 8: round 1 verifies itself): queued as tied, listed without a search, undecided by the FP64 keys too: exact.
    exact=False: the queries 2^-30, 2^-29, 2^-28 m off their lattice points — still exact numbers; the six distances now differ,
    by 1e-8 of themselves: FP32 keys tie as before (the same late list), FP64 orders them, so that the oracle's choice among them
    is no longer its tree's traversal order and a REGISTRATION of the scene can be held to the oracle's"""
    rng = np.random.default_rng(106)
    g = np.stack(np.meshgrid(np.arange(9) * 0.125, np.arange(9) * 0.125, np.arange(8) * 0.125, indexing="ij"), -1).reshape(-1, 3)
    tgt = g + np.array([2.0, -1.0, 0.5])
    # exact=False: only lattice points with at least five of their six neighbours (inner and face points). The sixth key, or the
    # fifth neighbour's, then ties with the selection's last in FP32 and the fit refuses WHATEVER order the tied keys came in;
    # an edge or corner point's selection is all of its tied neighbours, and verifiable when they happen to come in ascending order
    ijk = np.stack(np.meshgrid(np.arange(9), np.arange(9), np.arange(8), indexing="ij"), -1).reshape(-1, 3)
    inner = ((ijk == 0) | (ijk == np.array([8, 8, 7]))).sum(axis=1) <= 1
    pick = rng.choice(len(tgt), 300, replace=False) if exact else rng.choice(np.nonzero(inner)[0], 300, replace=False)
    src = tgt[pick] + (0.0 if exact else np.array([2.0 ** -30, 2.0 ** -29, 2.0 ** -28]))
    se, te = edge_pair(rng)
    return scene("lattice_k%d%s" % (k, "" if exact else "_off"), "plane", se, src, te, tgt, k_p=k, ties=exact)


def lean_limit(n):
    """the wall grown to n = 65 536 / 65 535 points at the same density (46.4 m x 17 m: h = 0.44 again) and 100 queries 0.55 - 0.8 m
    in front of it: one cell off the grid (out = 1: round 1 searches them) but the wall lies beyond the faces of their 3x3x3
    block: queued plain. At 65 535 points the lean 5x5x5 search takes them; at 65 536 positions no longer fit 16-bit halves
    and the rest kernel hands them straight on"""
    rng = np.random.default_rng(107)
    tgt = wall_points(rng, 65536, 46.4, 17.0)[:n]
    # (none of them within 3 m of the one point the twin lacks: r + 0.8 m, so that point is in no query's list)
    away = np.nonzero(np.linalg.norm(tgt[:65535] - wall_points(np.random.default_rng(107), 65536, 46.4, 17.0)[65535], axis=1) > 3.0)[0]
    src = tgt[rng.choice(away, 100, replace=False)] + np.column_stack([np.zeros(100), rng.uniform(0.55, 0.8, 100), np.zeros(100)])
    return scene("lean_limit_%d" % n, "plane", NONE, src, NONE, tgt)


def rod(k=5):
    """4 000 edge points along a 10 m rod of 3 x 3 mm (more than kBruteMax: the edge instantiations of the grid kernels and of
    the whole queue chain): area = 2 * (2 * 10 * 0.003) = 0.12, h = sqrt(8 * 0.12 / 4 000) = 0.0155 (above r / 1000), 646 x 1 x 1
    cells. ceil(r / h) + 1 = 66 > 64 shells and nx > 64: the cooperative search does not apply to any query. 100 queries 0.2 m
    off the rod (13 cells off the grid: queued plain, the 5x5x5 block misses the grid, listed) and 100 on it"""
    rng = np.random.default_rng(108)
    tgt = np.column_stack([rng.uniform(0.0, 10.0, 4000), rng.uniform(0, 0.003, 4000), rng.uniform(0, 0.003, 4000)]) + np.array([1.0, 2.0, 0.5])
    on = tgt[rng.choice(4000, 100, replace=False)] + rng.normal(size=(100, 3)) * 1e-4
    ang = rng.uniform(0, 2 * np.pi, 100)
    off = np.column_stack([rng.uniform(1.5, 10.5, 100), 2.0015 + 0.2 * np.cos(ang), 0.5015 + 0.2 * np.sin(ang)])
    return scene("rod", "edge", np.concatenate([on, off]), NONE, tgt, NONE, k_e=k)


BRUTE_SIZES = (1, 4, 255, 256, 257, 511, 512)  # kBruteTile = 256 and its pads, kBruteMax


def brute(n, k=5):
    """an edge target of n points on three lines (every third point a duplicate of its predecessor when n >= 4: exact ties)
    with ordinary queries and queries metres off the set's box (the FP32 stage does not apply); n < k: fewer points than k"""
    rng = np.random.default_rng(109 + n)
    t = rng.uniform(0.0, 1.5, (n, 1))
    d = np.array([[1.0, 0.1, 0.0], [0.0, 1.0, 0.2], [0.1, 0.0, 1.0]])[np.arange(n) % 3]
    tgt = np.array([2.0, -1.0, 1.5]) + t * d + rng.normal(size=(n, 3)) * 1e-3
    if n >= 4:
        tgt[2::3] = tgt[1::3][:len(tgt[2::3])]
    src = np.concatenate([tgt[rng.integers(0, n, 40)] + rng.normal(size=(40, 3)) * 5e-3, rng.uniform(-3, 3, (20, 3)) + np.array([2.0, -1.0, 1.5])])
    w = wall()
    return scene("brute_%d" % n, "edge", src, w.src_p, tgt, w.tgt_p, k_e=k, ties=n >= 4)


# ---- what the g++ build says about a scene ---------------------------------------------------------------------------------
_routes = {}


def routes(s, handoff):
    """hostcheck_lib.knn_routes of the scene's kind, once per (scene, k, form of round 1); read-only"""
    import hostcheck_lib as Hc
    q, t, k, r = sets(s)
    key = (s.name, s.kind, k, r, len(q), len(t), bool(handoff))
    if key not in _routes:
        _routes[key] = Hc.knn_routes(t, q, k, r, handoff)
    return _routes[key]


def expected(R, n_tgt, one_stage, coop):
    """the census's round-1 and queue counts for a scene whose routes (hostcheck_lib.knn_routes) are R, under a form of the chain:
    the pieces composed in the kernels' order (associate_knn_rest_kernel, the leftover kernel, the exact collector)"""
    r1, lean_set = R["r1"], n_tgt <= K_LEAN_MAX
    queued = r1 > 0
    wide, tied = r1 == WIDE, r1 == TIED
    searched = queued & (one_stage | (~tied & ((lean_set & ~wide) | (wide & (not coop)))))
    kept = np.full(len(r1), -1)
    kept = np.where(searched & wide, R["wide"], kept)
    if not one_stage:
        kept = np.where(searched & ~wide, R["lean2"], kept)
    else:
        kept = np.where(searched & (kept < 0), R["keyed"], kept)
    listed = queued & (kept < 0)
    exact = listed if one_stage else listed & (R["keyed"] < 0)
    before_fit = kept if one_stage else np.where(listed, R["keyed"], kept)
    return dict(verified=int((~queued & ~R["unverified"]).sum()), unverified=int(R["unverified"].sum()), queued=int(queued.sum()),
                queued_plain=int((r1 == PLAIN).sum()), queued_wide=int(wide.sum()), queued_tied=int(tied.sum()),
                rest_searched=int(searched.sum()), listed=int(listed.sum()), exact=int(exact.sum()),
                leftover_finished=int(listed.sum() - exact.sum()), late=int(R["refused"].sum()), late_min=int(R["refused_any_order"].sum()),
                _queued=queued, _after_rest=kept[queued], _before_fit=before_fit[queued])


# the counts that must EQUAL the g++ build's. `late` is not among them: whether the fit can verify a selection whose FP32 keys tie
# depends on the order of the tied candidates' running numbers, that is on the order of the target points inside a cell, which the
# device's target builds leave to their atomics (register_kernels.hip: grid_build_kernel). The g++ build gives its bounds: every
# selection it refuses whatever the order is late, and nothing is late that is not an unverified selection.
COUNTS = ("verified", "unverified", "queued", "queued_plain", "queued_wide", "queued_tied", "rest_searched", "listed", "exact",
          "leftover_finished")


def rest_blocks_one_pair(n_src):
    """workgroups of the queue kernels for ONE pair: 4096 wanted, capped at one pass over a full queue — the round-1 kernel's
    ceil(n_src / 256) workgroups of 256 threads, in workgroups of 64"""
    return min(4096, (n_src + 255) // 256 * 4)


def model_census(s, one_stage, coop, handoff=False):
    """a census as the g++ build says it should read (the fields check_census looks at), for the CPU tests"""
    import types
    q, t, k, r = sets(s)
    R = routes(s, handoff)
    e = expected(R, len(t), one_stage, coop)
    r1 = R["r1"][e["_queued"]]
    c = types.SimpleNamespace(**{n: e[n] for n in COUNTS + ("late",)})
    c.n_src, c.stride, c.queued_words = len(q), max(len(q), len(t)), e["queued"]
    c.one_stage, c.leftover_kernel, c.rest_blocks = int(one_stage), 0 if one_stage else (2 if coop else 1), rest_blocks_one_pair(len(q))
    c.lean_set = int(len(t) <= K_LEAN_MAX)
    c.entry_query = np.nonzero(e["_queued"])[0].astype(np.uint32)
    c.entry_reason = np.where(r1 == WIDE, REASON_WIDE, np.where(r1 == TIED, REASON_TIED, 0)).astype(np.uint32)
    c.count_after_rest, c.count_before_fit = e["_after_rest"].astype(np.int32), e["_before_fit"].astype(np.int32)
    c.late_query = np.nonzero(R["refused"])[0].astype(np.uint32)
    return c


# ---- the identities every census obeys -------------------------------------------------------------------------------------
def check_census(c):
    """c: a capi.AssocCensus (or anything with its fields). Raises AssertionError naming the identity that fails."""
    assert c.verified + c.unverified + c.queued_words == min(c.n_src, c.stride), "round-1 count words do not add up to the queries"
    assert c.queued_words == c.queued, "queued count words and the queue's length differ"
    assert c.queued_plain + c.queued_wide + c.queued_tied == c.queued, "reason bits do not add up to the queue"
    assert c.listed <= c.queued and c.exact <= c.listed and c.late <= c.unverified, "listed <= queued, exact <= listed, late <= unverified"
    assert c.leftover_finished == c.listed - c.exact, "leftover_finished"
    assert len(c.entry_reason) == c.queued
    assert len(c.late_query) == c.late == len(set(c.late_query.tolist())) and not np.isin(c.late_query, c.entry_query).any(), "late list: distinct, not queued"
    wide, tied = (c.entry_reason & REASON_WIDE) != 0, (c.entry_reason & REASON_TIED) != 0
    assert not (wide & tied).any() and int(wide.sum()) == c.queued_wide and int(tied.sum()) == c.queued_tied, "per-entry reason bits"
    assert int((c.count_after_rest < 0).sum()) == c.listed, "listed is not the number of entries the rest kernel left negative"
    assert int((c.count_before_fit < 0).sum()) == c.exact, "exact is not the number of entries negative in front of the queued fit"
    assert not ((c.count_after_rest >= 0) & (c.count_before_fit != c.count_after_rest)).any(), "a finished entry's count changed"
    if c.one_stage:
        assert c.exact == c.listed and c.rest_searched == c.queued and c.leftover_kernel == 0, "one stage: all searched, exact == listed"
    elif c.rest_blocks:
        coop = c.leftover_kernel == 2
        want = c.queued_plain * c.lean_set + c.queued_wide * (0 if coop else 1)
        assert c.rest_searched == want, "rest_searched against the reason bits, lean_set and the leftover kernel"
    else:
        assert c.queued == 0 and c.rest_searched == 0 and c.leftover_kernel == 0, "no queue chain: nothing queued"
    # an entry the rest kernel did not search is listed
    assert c.listed >= c.queued - c.rest_searched, "entries handed straight on are listed"
    assert len(set(c.entry_query.tolist())) == c.queued and (c.queued == 0 or int(c.entry_query.max()) < c.n_src), "queue entries: distinct queries"
