"""GPU parity, rows a16-a19 ONE BY ONE: the neighbour lists of knnSearch (order included), the
lines of fitLine and the planes of fitPlane as the association kernels produce them, against the oracle's own
functions — not through valid-sets and poses. Entry points: loamx_associate (one association pass of the registration
kernels, read out per source feature), loamx_knn_search, loamx_fit_lines, loamx_fit_planes (include/loamx.h).
Reference: kdtree.cpp:10-28, geometry.cpp:42-73, registration.cpp:23-103."""
import numpy as np
import pytest

import reference_kats as K
from gpu_common import ctx, option, pose_diff, to_capi_reg
from loam_amd import capi

pytestmark = pytest.mark.gpu

IDENT = np.array([0, 0, 0, 1.0, 0, 0, 0])

# Worst observed (fit error / allowance) per kind over everything this module checks: the allowances
# widen with the conditioning of a point set, so a regression INSIDE an allowance would pass silently. The last test of
# the module writes the table to gpurun_out/fit_error_vs_allowance.json and holds the well-conditioned sets (the bench
# scans) to the plain bar.
WORST = {}


def note_ratio(kind, err, allowance, where):
    r = float(err) / float(allowance)
    if r > WORST.get(kind, (-1.0, None, 0.0, 0.0))[0]:
        WORST[kind] = (r, str(where), float(err), float(allowance))


def line_tol(pts):
    """what two correct eigen-solvers may differ by on this point set: rounding x conditioning of the top eigenvector"""
    c = pts - pts.mean(axis=0)
    w = np.linalg.eigvalsh(c.T @ c)
    gap = max(w[2] - w[1], 1e-300)
    return 1e-12 + 4e-16 * max(w[2], 1e-300) / gap * (1.0 + np.abs(pts).max())


def check_kind(oracle, name, dump, src, tgt, pose, is_plane, oreg, ties=False):
    d = dump["plane" if is_plane else "edge"]
    k = oreg.num_plane_neighbors if is_plane else oreg.num_edge_neighbors
    radius = oreg.max_plane_neighbor_dist if is_plane else oreg.max_edge_neighbor_dist
    if len(src) == 0:
        return 0
    if len(tgt) == 0:
        assert not d["valid"].any() and all(len(x) == 0 for x in d["nn"])
        return 0
    valid, nearest, moved, prims = oracle.associate(src, tgt, pose, is_plane, oreg)
    assert np.array_equal(d["valid"], valid), name
    assert np.abs(d["moved"] - moved).max() <= 1e-12 * (1.0 + np.abs(moved).max()), name
    tree = oracle.KDTree(tgt)
    checked = 0
    for i in range(len(src)):
        want = tree.knn(moved[i], k, radius)
        got = d["nn"][i]
        assert len(got) == len(want), (name, i)
        if not np.array_equal(got, want.astype(np.uint32)):
            # equal distances (lattice scenes): nanoflann's order among ties is its traversal order;
            # the distances themselves must be the same numbers in the same order
            assert ties, (name, i, got, want)
            dg = ((tgt[got] - moved[i]) ** 2).sum(axis=1)
            dw = ((tgt[want.astype(np.int64)] - moved[i]) ** 2).sum(axis=1)
            assert np.array_equal(dg, dw), (name, i)
            continue
        if valid[i]:
            assert got[0] == nearest[i]
            err = np.abs(d["prim"][i] - prims[i]).max()
            kind = ("plane " if is_plane else "line ") + name.split()[0]
            if err > 1e-12:  # (the conditioning of the point set, computed only when the plain bar is missed)
                nb = tgt[got]
                if is_plane:
                    allow = 1e-12 * (1.0 + np.linalg.cond(nb) ** 2 * 1e-3)
                    note_ratio(kind + " (cond^2 allowance)", err, allow, (name, i))
                    assert err <= allow, (name, i)
                else:
                    a, b, oa, ob = d["prim"][i, :3], d["prim"][i, 3:], prims[i, :3], prims[i, 3:]
                    flip = max(np.abs(a - ob).max(), np.abs(b - oa).max())  # (the direction's sign: the residual is symmetric in a, b)
                    note_ratio(kind + " (eigen-gap allowance)", min(err, flip), line_tol(nb), (name, i))
                    assert min(err, flip) <= line_tol(nb), (name, i, err, flip)
            else:
                note_ratio(kind + " (plain 1e-12 bar)", err, 1e-12, (name, i))
            checked += 1
    return checked


@pytest.mark.parametrize("H,W,seed,pair", [(64, 1024, 20240311, 0), (64, 1024, 7, 1), (32, 512, 3, 2)])
def test_associate_lists_and_fits_on_scan_pairs(oracle, H, W, seed, pair):
    """the bench workload's pairs: every plane / edge query's neighbour list in order, every line and plane"""
    A = capi.synth_scan_host(seed, pair, 0, H, W, 0.01)
    B = capi.synth_scan_host(seed, pair, 1, H, W, 0.01)
    ea, pa = oracle.extract_features(A, H, W, 1.0, 120.0)
    eb, pb = oracle.extract_features(B, H, W, 1.0, 120.0)
    oreg = oracle.RegParams()
    # at the identity (first ICF iteration) and at the oracle's estimate after one iteration (second iteration's input)
    _, _, _, info = oracle.register_features(B[eb], B[pb], A[ea], A[pa], want_info=True)
    est1 = oracle.pose_compose(np.array(list(info[0].update)), IDENT)
    for pose in (IDENT, est1):
        dump = ctx().associate(B[eb], B[pb], A[ea], A[pa], pose)
        ne = check_kind(oracle, "scan-edge", dump, B[eb], A[ea], pose, False, oreg)
        npl = check_kind(oracle, "scan-plane", dump, B[pb], A[pa], pose, True, oreg)
        assert ne > 50 and npl > 2000


def test_every_per_kind_parameter_different_under_poison(oracle):
    """k, radius and the fewest fit points all differ between edges and planes (min_plane_fit_points off its default as
    well), scratch starting as 0xFF bytes: a parameter or buffer of one kind read for the other shows in the lists, the
    valid sets or the iteration counts."""
    H, W, seed, pair = 32, 512, 3, 2
    A = capi.synth_scan_host(seed, pair, 0, H, W, 0.01)
    B = capi.synth_scan_host(seed, pair, 1, H, W, 0.01)
    ea, pa = oracle.extract_features(A, H, W, 1.0, 120.0)
    eb, pb = oracle.extract_features(B, H, W, 1.0, 120.0)
    oreg = oracle.RegParams()
    oreg.num_edge_neighbors, oreg.num_plane_neighbors = 3, 7
    oreg.max_edge_neighbor_dist, oreg.max_plane_neighbor_dist = 0.6, 1.5
    oreg.min_line_fit_points, oreg.min_plane_fit_points = 2, 6
    reg = to_capi_reg(oreg)
    # not vacuous: both kinds associate, and in both the oracle turns a query away for too few neighbours inside the radius
    for src, tgt, is_plane in ((B[eb], A[ea], False), (B[pb], A[pa], True)):
        valid, _, moved, _ = oracle.associate(src, tgt, IDENT, is_plane, oreg)
        tree = oracle.KDTree(tgt)
        k, radius, fewest = (7, 1.5, 6) if is_plane else (3, 0.6, 2)
        assert valid.sum() >= 20 and any(len(tree.knn(m, k, radius)) < fewest for m in moved)
    po, to, io, info = oracle.register_features(B[eb], B[pb], A[ea], A[pa], params=oreg, want_info=True)
    with option("DEBUG_POISON"):
        dump = ctx().associate(B[eb], B[pb], A[ea], A[pa], IDENT, reg)
        pg, tg, ig, det = ctx().register_features(B[eb], B[pb], A[ea], A[pa], reg=reg, want_detail=True)
    assert check_kind(oracle, "scan-edge", dump, B[eb], A[ea], IDENT, False, oreg) >= 20
    assert check_kind(oracle, "scan-plane", dump, B[pb], A[pa], IDENT, True, oreg) >= 20
    assert (tg, ig) == (to, io)
    assert [(a.n_edge_assoc, a.n_plane_assoc) for a in info] == [(d["n_edge"], d["n_plane"]) for d in det["iterations"]]
    rot, trans = pose_diff(oracle, po, pg)
    assert rot < 1e-5 and trans < 1e-5, (rot, trans)  # (SE3_TOL of test_gpu_register.py)
    for pairs, src, tgt, is_plane in ((det["iterations"][0]["edge_pairs"], B[eb], A[ea], False),
                                      (det["iterations"][0]["plane_pairs"], B[pb], A[pa], True)):
        valid, nearest, _, _ = oracle.associate(src, tgt, IDENT, is_plane, oreg)
        assert np.array_equal(pairs[:, 0], np.nonzero(valid)[0]) and np.array_equal(pairs[:, 1], nearest[valid])


def test_associate_does_not_depend_on_max_iterations(oracle):
    """associateEdges / associatePlanes (registration.cpp:23-103) know nothing of max_iterations; with
    max_iterations = 0 the pair was never active and the dump read workspace nobody had written."""
    H, W = 16, 256
    A = capi.synth_scan_host(11, 0, 0, H, W, 0.01)
    B = capi.synth_scan_host(11, 0, 1, H, W, 0.01)
    ea, pa = oracle.extract_features(A, H, W, 1.0, 120.0)
    eb, pb = oracle.extract_features(B, H, W, 1.0, 120.0)
    c = ctx()
    want = c.associate(B[eb], B[pb], A[ea], A[pa], IDENT)
    reg0 = capi.RegistrationParams()
    reg0.max_iterations = 0
    with option("DEBUG_POISON"):
        got = c.associate(B[eb], B[pb], A[ea], A[pa], IDENT, reg0)
    for kind in ("edge", "plane"):
        assert np.array_equal(got[kind]["valid"], want[kind]["valid"])
        assert all(np.array_equal(a, b) for a, b in zip(got[kind]["nn"], want[kind]["nn"]))
        assert np.array_equal(got[kind]["prim"], want[kind]["prim"]) and np.array_equal(got[kind]["moved"], want[kind]["moved"])
    assert want["plane"]["valid"].sum() > 100


def test_associate_on_the_reference_scene_with_ties(oracle):
    """tests/test_registration.cpp:8-56: regular 0.05 m grids, every query has equidistant neighbours"""
    tgt_e, tgt_p = K.registration_scene()
    case = K.REGISTRATION_CASES[1]
    src_e = K.transform_points(case["source_T_target"], tgt_e)
    src_p = K.transform_points(case["source_T_target"], tgt_p)
    pose = IDENT if case["init"] is None else np.asarray(case["init"], dtype=np.float64)
    oreg = oracle.RegParams()
    for stage in ("QUEUE_ONE_STAGE", "QUEUE_TWO_STAGE"):
        with option(stage):
            dump = ctx().associate(src_e, src_p, tgt_e, tgt_p, pose)
        check_kind(oracle, "edge " + stage, dump, src_e, tgt_e, pose, False, oreg, ties=True)
        check_kind(oracle, "plane " + stage, dump, src_p, tgt_p, pose, True, oreg, ties=True)


@pytest.mark.parametrize("seed", range(40))
def test_associate_fuzz_lists_and_fits(oracle, seed):
    """random clouds (planes, lines, blobs, sparse shells, anisotropic lattices), random k and radii, sets on both sides
    of the brute-force / grid / queue thresholds"""
    rng = np.random.default_rng(7000 + seed)

    def cloud(n):
        kind = rng.integers(0, 5)
        if kind == 0:
            o, u, v = rng.normal(size=3) * 3, rng.normal(size=3), rng.normal(size=3)
            pts = o + np.outer(rng.uniform(-4, 4, n), u / np.linalg.norm(u)) + np.outer(rng.uniform(-4, 4, n), v / np.linalg.norm(v))
            pts += rng.normal(size=pts.shape) * 0.01
        elif kind == 1:
            pts = np.concatenate([rng.normal(size=3) * 4 + np.outer(np.linspace(-3, 3, max(2, n // 3)), rng.normal(size=3)) for _ in range(3)])[:n]
            pts = pts + rng.normal(size=pts.shape) * 0.004
        elif kind == 2:
            pts = rng.normal(size=(n, 3)) * rng.uniform(0.3, 5.0)
        elif kind == 3:
            d = rng.normal(size=(n, 3))
            pts = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(5, 30)
            pts[: n // 10] = rng.normal(size=(n // 10, 3)) * 0.2 + 100.0
        else:
            g = int(round(n ** (1 / 3))) + 1
            pts = np.stack(np.meshgrid(np.arange(g) * 0.25, np.arange(g) * 0.27, np.arange(g) * 0.31), -1).reshape(-1, 3)[:n]
        return np.ascontiguousarray(pts + rng.normal(size=3)), kind == 4

    n_e, n_p = int(rng.choice([0, 3, 7, 60, 400, 700])), int(rng.choice([4, 9, 150, 2000, 6000]))
    (tgt_e, tie_e), (tgt_p, tie_p) = (cloud(n_e) if n_e else (np.zeros((0, 3)), False)), cloud(n_p)
    ax = rng.normal(size=3)
    T = K.pose7(K.quat_angle_axis(rng.uniform(0, 0.05), ax / np.linalg.norm(ax)), rng.normal(size=3) * 0.05)
    src_e = K.transform_points(T, tgt_e[rng.random(len(tgt_e)) < 0.8]) if len(tgt_e) else tgt_e
    src_p = K.transform_points(T, tgt_p[rng.random(len(tgt_p)) < 0.8])
    src_e = src_e + rng.normal(size=src_e.shape) * 0.003
    src_p = src_p + rng.normal(size=src_p.shape) * 0.003
    reg, oreg = capi.RegistrationParams(), oracle.RegParams()
    reg.num_edge_neighbors = oreg.num_edge_neighbors = int(rng.choice([2, 3, 5, 8, 11]))
    reg.num_plane_neighbors = oreg.num_plane_neighbors = int(rng.choice([4, 5, 7, 8, 12, 16]))
    reg.min_line_fit_points = oreg.min_line_fit_points = int(rng.choice([2, 3]))
    reg.max_plane_neighbor_dist = oreg.max_plane_neighbor_dist = float(rng.choice([0.5, 2.0, -1.0]))
    reg.max_edge_neighbor_dist = oreg.max_edge_neighbor_dist = float(rng.choice([0.3, 1.0, -1.0]))
    pose = K.pose7(K.quat_angle_axis(rng.uniform(0, 0.02), ax / np.linalg.norm(ax)), rng.normal(size=3) * 0.02)
    # both forms of the queue chain: small batches take the one-stage form by themselves, the two-stage form (lean search
    # of the 5x5x5 block, then the listed leftovers) is what 1 024-pair batches run
    for stage in ("QUEUE_ONE_STAGE", "QUEUE_TWO_STAGE"):
        with option(stage):
            dump = ctx().associate(src_e, src_p, tgt_e, tgt_p, pose, reg)
        check_kind(oracle, f"edge {seed} {stage}", dump, src_e, tgt_e, pose, False, oreg, ties=tie_e)
        check_kind(oracle, f"plane {seed} {stage}", dump, src_p, tgt_p, pose, True, oreg, ties=tie_p)


@pytest.mark.parametrize("case", ["dense", "isolated", "no_radius", "mixed"])
def test_cooperative_leftover_search_on_the_queries_it_exists_for(oracle, case):
    """associate_knn_coop_kernel (round 4): one wavefront per listed leftover of the queue. Scenes made of the leftovers it
    exists for — dense blocks (more than 63 batches in the 3x3x3 block: wide running numbers), isolated queries (the
    radius cube, shell by shell), a search without a radius (not applicable: lane 0 falls back to the one-lane search),
    and a mix with exact ties — for k = 5, 8 and 16, against the oracle's KD-tree lists and fits; the one-lane leftover
    kernel (NO_COOP_LEFT) must produce the same dump."""
    rng = np.random.default_rng({"dense": 1, "isolated": 2, "no_radius": 3, "mixed": 4}[case])
    if case == "dense":      # ~25 000 points in a 1.2 m cube inside a 100 m bounding box (three outliers): the cell table's cap
        # makes the cells 2.5 m wide, so every 3x3x3 block around the cube holds all of it
        tgt_p = np.concatenate([rng.uniform(-0.6, 0.6, (25000, 3)) + np.array([3.0, -2.0, 1.0]), [[50.0, 50, 50], [-50, -50, -50], [50, -50, 0]]])
        src_p = tgt_p[rng.choice(len(tgt_p), 1500, replace=False)] + rng.normal(size=(1500, 3)) * 0.01
        radius = 2.0
    elif case == "isolated":  # a sparse shell: most queries find fewer than k points within the radius, many none in 5x5x5
        tgt_p = rng.uniform(-15, 15, (3000, 3))
        src_p = rng.uniform(-15, 15, (1200, 3))
        radius = 2.0
    elif case == "no_radius":
        tgt_p = rng.uniform(-10, 10, (2500, 3))
        src_p = rng.uniform(-40, 40, (600, 3))  # (most queries lie cells away from the grid: neither lean search applies)
        radius = -1.0
    else:                     # a dense wall, a sparse room, and a lattice (equidistant neighbours)
        wall = np.column_stack([rng.uniform(-4, 4, 12000), np.full(12000, 5.0) + rng.normal(size=12000) * 0.003, rng.uniform(-1, 2, 12000)])
        room = rng.uniform(-8, 8, (1500, 3))
        g = np.stack(np.meshgrid(np.arange(12) * 0.2, np.arange(12) * 0.2, np.arange(12) * 0.2), -1).reshape(-1, 3) + np.array([-6.0, -6.0, -1.0])
        tgt_p = np.concatenate([wall, room, g])
        src_p = np.concatenate([wall[::10] + rng.normal(size=(1200, 3)) * 0.01, rng.uniform(-8, 8, (500, 3)), g[::3] + 0.05])
        radius = 1.5
    tgt_p, src_p = np.ascontiguousarray(tgt_p), np.ascontiguousarray(src_p)
    none = np.zeros((0, 3))
    for k in (5, 8, 16):
        reg, oreg = capi.RegistrationParams(), oracle.RegParams()
        reg.num_plane_neighbors = oreg.num_plane_neighbors = k
        reg.max_plane_neighbor_dist = oreg.max_plane_neighbor_dist = radius
        with option("QUEUE_TWO_STAGE"):
            dump = ctx().associate(none, src_p, none, tgt_p, IDENT, reg)
            cen = ctx().last_assoc_census("plane")
            with option("NO_COOP_LEFT"):
                lanes = ctx().associate(none, src_p, none, tgt_p, IDENT, reg)
                cen_lanes = ctx().last_assoc_census("plane")
        queued, listed = dump["plane"]["queued"]
        assert queued > 20 and listed > 5, (case, k, queued, listed)  # (the leftover kernel really had work)
        # ... and it was the kernel meant (the census): the cooperative one, but the one-lane kernel where there is no
        # radius (the launcher does not start the cooperative kernel for such a search at all), and finished what was listed
        want = capi.ASSOC_LEFTOVER_COOP if radius > 0 else capi.ASSOC_LEFTOVER_LEFT
        assert (cen.leftover_kernel, cen.one_stage, cen.queued, cen.listed) == (want, 0, queued, listed), (case, k, cen)
        assert cen.leftover_finished + cen.exact == listed
        assert (cen_lanes.leftover_kernel, cen_lanes.one_stage) == (capi.ASSOC_LEFTOVER_LEFT, 0)
        check_kind(oracle, f"plane coop-{case}-{k}", dump, src_p, tgt_p, IDENT, True, oreg, ties=(case == "mixed"))
        assert all(np.array_equal(a, b) for a, b in zip(dump["plane"]["nn"], lanes["plane"]["nn"])) or case == "mixed"
        assert np.array_equal(dump["plane"]["valid"], lanes["plane"]["valid"])


def test_fit_entry_points_against_the_oracle(oracle):
    """geometry_internal::fitLine / fitPlane (geometry.h:102, :123) through loamx_fit_lines / loamx_fit_planes: every k
    the reference accepts up to 32, including the k > 8 route the association kernels never take"""
    rng = np.random.default_rng(11)
    for k in (2, 3, 4, 5, 8, 9, 20, 32):
        n = 200
        o = rng.normal(size=(n, 1, 3)) * 5
        u = rng.normal(size=(n, 1, 3))
        line_pts = o + rng.uniform(-1, 1, (n, k, 1)) * u / np.linalg.norm(u, axis=2, keepdims=True) + rng.normal(size=(n, k, 3)) * 0.01
        a, b, cond = ctx().fit_lines(line_pts)
        assert (cond == np.finfo(np.float64).max).all()  # geometry.cpp:55-56
        for i in range(n):
            oa, ob, oc = oracle.fit_line(line_pts[i])
            tol = line_tol(line_pts[i])
            assert min(max(np.abs(a[i] - oa).max(), np.abs(b[i] - ob).max()), max(np.abs(a[i] - ob).max(), np.abs(b[i] - oa).max())) <= tol, (k, i)
        if k < 3:
            continue
        v = rng.normal(size=(n, 1, 3))
        plane_pts = o + rng.uniform(-1, 1, (n, k, 1)) * u + rng.uniform(-1, 1, (n, k, 1)) * v + rng.normal(size=(n, k, 3)) * 0.005
        nrm, d, avg = ctx().fit_planes(plane_pts)
        for i in range(n):
            on, od, oavg = oracle.fit_plane(plane_pts[i])
            tol = 1e-12 * (1.0 + np.linalg.cond(plane_pts[i]) ** 2 * 1e-3)
            assert np.abs(nrm[i] - on).max() <= tol and abs(d[i] - od) <= tol * (1 + abs(od)) and abs(avg[i] - oavg) <= tol, (k, i)
    with pytest.raises(capi.LoamxError):
        ctx().fit_lines(np.zeros((1, 1, 3)))
    with pytest.raises(capi.LoamxError):
        ctx().fit_planes(np.zeros((1, 33, 3)))


def test_fits_are_bit_identical_to_the_host_build_of_the_same_header():
    """The kernels' fit_line / fit_plane against the g++ build of the same header (tests/hostcheck), bit for bit: the
    device's division and square-root sequences — including the reciprocal that divisions by one divisor share in
    fit_plane — round exactly as IEEE division does. Sets of every scale, near-degenerate and exactly degenerate."""
    import hostcheck_lib as Hc
    rng = np.random.default_rng(5)
    sets = []
    for k in (3, 4, 5, 7, 8):
        n = 1500
        o = rng.normal(size=(n, 1, 3)) * 5
        u, v = rng.normal(size=(n, 1, 3)), rng.normal(size=(n, 1, 3))
        flat = o + rng.uniform(-1, 1, (n, k, 1)) * u + rng.uniform(-1, 1, (n, k, 1)) * v + rng.normal(size=(n, k, 3)) * 10.0 ** rng.integers(-9, 0, (n, 1, 1))
        scale = np.where(rng.random((n, 1, 1)) < 0.2, 10.0 ** rng.integers(-140, 140, (n, 1, 1)), 10.0 ** rng.integers(-3, 4, (n, 1, 1)))
        pts = flat * scale
        lattice = np.round(rng.normal(size=(200, k, 3)) * 2) * 0.25 + 2.0   # exact ties, zero columns, collinear sets
        axis = np.zeros((50, k, 3))
        axis[:, :, 0] = rng.normal(size=(50, k))                            # rank 1: two zero columns
        sets.append(np.concatenate([pts, lattice, axis]))
    for pts in sets:
        k = pts.shape[1]
        nrm, d, avg = ctx().fit_planes(pts)
        a, b, _ = ctx().fit_lines(pts)
        bad = 0
        for i in range(len(pts)):
            hn, hd, havg = Hc.fit_plane(pts[i])
            got = np.array([*nrm[i], d[i], avg[i]])
            want = np.array([*hn, hd, havg])
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)) or (np.isnan(got) == np.isnan(want)).all() and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)]), (k, i, got, want)
            ha, hb = Hc.fit_line(pts[i])
            gl, wl = np.array([*a[i], *b[i]]), np.array([*ha, *hb])
            bad += not (np.array_equal(gl, wl) or (np.isnan(gl).any() and np.isnan(wl).any()))
        assert bad == 0, (k, bad)


def test_fit_line_entry_point_on_degenerate_lattices(oracle):
    """neighbours on a lattice: covariance exactly diagonal with two EQUAL eigenvalues — "the" direction is the one
    Eigen's selection sort leaves last (oracle symeig3 / reg_math.h fit_line)"""
    for s in ([0.25, 0.0, 0.0], [0.0, 0.5, 0.0], [0.0, 0.0, 0.125]):
        for t in ([0.25, 0.0, 0.0], [0.0, 0.5, 0.0], [0.0, 0.0, 0.125]):
            pts = np.array([[0, 0, 0], s, [-x for x in s], t, [-x for x in t]], dtype=np.float64) + 2.0
            a, b, _ = ctx().fit_lines(pts[None])
            oa, ob, _ = oracle.fit_line(pts)
            assert (np.array_equal(a[0], oa) and np.array_equal(b[0], ob)) or (np.array_equal(a[0], ob) and np.array_equal(b[0], oa)), (s, t)


def test_knn_entry_point_against_the_oracle_tree(oracle):
    """kdtree_internal::knnSearch (kdtree.h:49) through loamx_knn_search on a target index: index lists in order for
    k = 1..16, with and without the radius, queries inside, outside and far from the set; the empty set"""
    rng = np.random.default_rng(3)
    c = ctx()
    for n, scale in ((37, 1.0), (600, 3.0), (30000, 8.0)):
        pts = rng.normal(size=(n, 3)) * scale
        index = c.target_index(pts[: n // 3], pts)  # edge set = a third of the points, planar set = all of them
        tree_p, tree_e = oracle.KDTree(pts), oracle.KDTree(pts[: n // 3])
        q = np.concatenate([pts[rng.integers(0, n, 150)] + rng.normal(size=(150, 3)) * 0.05, rng.normal(size=(40, 3)) * scale * 3,
                            np.array([[1e3, -1e3, 5e2]])])
        for k in (1, 3, 5, 8, 13, 16):
            for radius in (-1.0, 0.4 * scale, 0.02):
                got = c.knn_search(index, 1, q, k, radius)
                for i in range(len(q)):
                    assert np.array_equal(got[i], tree_p.knn(q[i], k, radius).astype(np.uint32)), (n, k, radius, i)
        got = c.knn_search(index, 0, q, 5, -1.0)
        for i in range(len(q)):
            assert np.array_equal(got[i], tree_e.knn(q[i], 5, -1.0).astype(np.uint32))
        c.target_index_destroy(index)
    index = c.target_index(np.zeros((0, 3)), np.zeros((0, 3)))
    assert all(len(x) == 0 for x in c.knn_search(index, 1, rng.normal(size=(5, 3)), 5))  # tests/test_registration.cpp:177-199
    with pytest.raises(capi.LoamxError):
        c.knn_search(index, 1, np.zeros((1, 3)), 17)
    c.target_index_destroy(index)


def test_zz_worst_fit_error_against_its_allowance():
    """runs last in this module: the table of worst (error / allowance) ratios, written for the round's record"""
    import json
    import os
    if not WORST:
        pytest.skip("no fits were checked in this session")
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    os.makedirs(out, exist_ok=True)
    table = {k: dict(ratio=v[0], where=v[1], error=v[2], allowance=v[3]) for k, v in sorted(WORST.items())}
    with open(os.path.join(out, "fit_error_vs_allowance.json"), "w") as f:
        json.dump(table, f, indent=1)
    print(json.dumps(table))
    assert all(v[0] <= 1.0 for v in WORST.values())
    # the bench scans' neighbourhoods are well conditioned: nothing there may need an allowance beyond 100x the plain bar
    for k, v in WORST.items():
        if k.startswith(("plane scan", "line scan")) and "plain" not in k:
            assert v[3] <= 1e-10, (k, v)
