"""GPU: the hand-off between the plane round-1 k-NN kernel and the plane fit of the mixed association launch (small edge
sets by brute force + planar sets through their grids, five neighbours: what scan pairs run). The round-1 kernel selects
the neighbours from its FP32 keys and leaves the moved query point in the record; the fit verifies the selection on the
FP64 points it gathers anyway, and what it refuses goes through a late list to associate_fit_late_kernel (exact search +
fit). The context option FORCE_LATE_VERIFY refuses every selection, so that every query the fit would have verified takes the
late list instead: same results, bit for bit.
  * association of one 16 x 256 scan pair (planar target sets of ~950 points: above the 512-point brute-force limit) against
    the oracle: neighbour lists in order, planes, lines, validity;
  * the tie path: a 9 x 9 x 8 lattice at 0.1 m as planar target, queries a tenth of a micron off lattice points (FP32 keys
    cannot order the six neighbours at 0.1 m, FP64 distances can: every selection is refused by the fit), 300 and 257 of
    them; association and register_features against the oracle;
  * a batch of 9 pairs (more than one group of eight) against the same pairs registered one by one: identical records."""
import numpy as np
import pytest

import reference_kats as K
from gpu_common import ctx, option, pose_diff
from loam_amd import capi
from test_gpu_direct import check_kind

pytestmark = pytest.mark.gpu

IDENT = np.array([0, 0, 0, 1.0, 0, 0, 0])
SE3_TOL = 1e-5  # (tests/test_gpu_register.py)
H, W, SEED = 16, 256, 11


def same_dump(a, b):
    for kind in ("edge", "plane"):
        assert np.array_equal(a[kind]["valid"], b[kind]["valid"])
        assert all(np.array_equal(x, y) for x, y in zip(a[kind]["nn"], b[kind]["nn"]))
        assert np.array_equal(a[kind]["prim"], b[kind]["prim"]) and np.array_equal(a[kind]["moved"], b[kind]["moved"])


def test_association_of_a_small_scan_pair(oracle):
    A = capi.synth_scan_host(SEED, 0, 0, H, W, 0.01)
    B = capi.synth_scan_host(SEED, 0, 1, H, W, 0.01)
    ea, pa = oracle.extract_features(A, H, W, 1.0, 120.0)
    eb, pb = oracle.extract_features(B, H, W, 1.0, 120.0)
    assert len(pa) > 512 >= len(ea) > 0  # the mixed launch: planar set through its grid, edge set by brute force
    oreg = oracle.RegParams()
    dump = ctx().associate(B[eb], B[pb], A[ea], A[pa], IDENT)
    assert check_kind(oracle, "scan-edge", dump, B[eb], A[ea], IDENT, False, oreg) > 10
    assert check_kind(oracle, "scan-plane", dump, B[pb], A[pa], IDENT, True, oreg) > 300
    with option("FORCE_LATE_VERIFY"):
        late = ctx().associate(B[eb], B[pb], A[ea], A[pa], IDENT)
    same_dump(dump, late)


def lattice_scene(n_src):
    rng = np.random.default_rng(257)
    g = np.stack(np.meshgrid(np.arange(9) * 0.1, np.arange(9) * 0.1, np.arange(8) * 0.1, indexing="ij"), -1).reshape(-1, 3)
    tgt_p = np.ascontiguousarray(g + np.array([2.0, -1.0, 0.5]))
    assert len(tgt_p) == 648
    pick = rng.choice(len(tgt_p), n_src, replace=False)
    on_p = tgt_p[pick] + rng.uniform(-1e-7, 1e-7, (n_src, 3))
    # three edges (lines in general position) next to the lattice, so that both kinds are there
    t = np.linspace(0.0, 1.5, 30)[:, None]
    tgt_e = np.concatenate([np.array([2.0, -1.0, 1.5]) + t * np.array([1.0, 0.1, 0.0]), np.array([3.2, -1.0, 0.4]) + t * np.array([0.0, 1.0, 0.2]),
                            np.array([1.8, 0.2, 0.5]) + t * np.array([0.1, 0.0, 1.0])])
    on_e = tgt_e[::2] + rng.normal(size=(len(tgt_e[::2]), 3)) * 1e-3
    T = K.pose7(K.quat_angle_axis(0.03, np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])), np.array([0.05, -0.02, 0.03]))
    return tgt_e, tgt_p, on_e, on_p, np.asarray(T, dtype=np.float64)


@pytest.mark.parametrize("n_src", [300, 257])
def test_tie_path_on_the_lattice(oracle, n_src):
    tgt_e, tgt_p, on_e, on_p, T = lattice_scene(n_src)
    Tinv = np.asarray(oracle.pose_inverse(T))
    src_e = np.ascontiguousarray([oracle.pose_act(Tinv, x) for x in on_e])
    src_p = np.ascontiguousarray([oracle.pose_act(Tinv, x) for x in on_p])
    oreg = oracle.RegParams()
    # the queries at `T` sit on the lattice points again (within the transform's rounding): lists against the oracle's KD-tree
    dump = ctx().associate(src_e, src_p, tgt_e, tgt_p, T)
    assert check_kind(oracle, "lattice-plane", dump, src_p, tgt_p, T, True, oreg) > n_src // 2
    check_kind(oracle, "lattice-edge", dump, src_e, tgt_e, T, False, oreg)
    with option("FORCE_LATE_VERIFY"):  # every query on the late list: the same dump
        late = ctx().associate(src_e, src_p, tgt_e, tgt_p, T)
    same_dump(dump, late)
    po, to, io, info = oracle.register_features(src_e, src_p, tgt_e, tgt_p, init_pose=T, want_info=True)
    pg, tg, ig, det = ctx().register_features(src_e, src_p, tgt_e, tgt_p, init_pose=T, want_detail=True)
    assert (tg, ig) == (to, io)
    assert [(a.n_edge_assoc, a.n_plane_assoc) for a in info] == [(d["n_edge"], d["n_plane"]) for d in det["iterations"]]
    assert info[0].n_plane_assoc > n_src // 2
    rot, trans = pose_diff(oracle, po, pg)
    assert rot < SE3_TOL and trans < SE3_TOL, (rot, trans)
    with option("FORCE_LATE_VERIFY"):
        pl, tl, il = ctx().register_features(src_e, src_p, tgt_e, tgt_p, init_pose=T)
    assert (tl, il) == (tg, ig) and np.array_equal(np.asarray(pl), np.asarray(pg))


def test_batch_of_nine_equals_the_pairs_one_by_one():
    c = ctx()
    P, N = 9, H * W
    lidar = capi.LidarParams(H, W, 1.0, 120.0)
    d_xyz, d_res = c.alloc(P * 2 * N * 24), c.alloc(P * 64)
    c.synth_scan_pairs_dev(SEED, 0, P, H, W, 0.01, d_xyz.ptr)

    def run(ptr, n):
        c.register_scan_pairs_dev(ptr, n, lidar, capi.FeatureExtractionParams(), capi.RegistrationParams(), d_res.ptr)
        c.synchronize()
        return d_res.download(np.uint8, n * 64).copy()

    whole = run(d_xyz.ptr, P)
    singles = np.concatenate([run(d_xyz.ptr + p * 2 * N * 24, 1) for p in range(P)])
    assert np.array_equal(whole, singles)
    rec = whole.view(capi.RESULT_DTYPE)
    assert (rec["iterations"] >= 2).all()  # (registrations that ran: more than one association pass each)
    with option("FORCE_LATE_VERIFY"):
        assert np.array_equal(run(d_xyz.ptr, P), whole)
