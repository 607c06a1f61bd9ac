"""GPU: the registration information matrix (include/loamx.h: loamx_reg_information) against its model.

The model: Context.associate at the same pose gives `valid`, `moved` and `prim` of every source feature — the bytes
information_kernel reads. The g++ build of info_math.h (tests/hostcheck_info) turns each valid record into its scaled row,
and the terms are summed exactly (math.fsum). The GPU may differ from that only by the order of its sums:
|got - want| <= n 2^-52 sum |term| per entry (recursive summation in any order), equal counters, a bitwise symmetric matrix;
the eigenpairs are judged on the GPU's own matrix by the residual rule of tests/info_common.py. Every case first asserts
from the model that it is not vacuous."""
import functools

import numpy as np
import pytest

import info_common as I
import reference_kats as K
from gpu_common import ctx
from loam_amd import capi

pytestmark = pytest.mark.gpu

IDENT = np.array([0, 0, 0, 1.0, 0, 0, 0])


@functools.lru_cache(maxsize=None)
def room(oracle, H, W, seed=3, pair=2):
    """(src_edge, src_planar, tgt_edge, tgt_planar, the oracle's registered pose) of one synthetic room pair"""
    A, B = capi.synth_scan_host(seed, pair, 0, H, W, 0.01), capi.synth_scan_host(seed, pair, 1, H, W, 0.01)
    ea, pa = oracle.extract_features(A, H, W, 1.0, 120.0)
    eb, pb = oracle.extract_features(B, H, W, 1.0, 120.0)
    sets = tuple(np.ascontiguousarray(x) for x in (B[eb], B[pb], A[ea], A[pa]))
    pose, _, _ = oracle.register_features(*sets)
    return sets + (np.asarray(pose, dtype=np.float64),)


def record_and_model(sets, pose, what):
    c = ctx()
    info = c.registration_information(*sets, pose=pose)
    m = I.model(*I.records_of_dump(c.associate(*sets, pose)))
    I.check_against_model(info, m, what)
    I.check_eigenpairs(info.information, info.eigenvalues, info.eigenvectors, what)
    return info, m


@pytest.mark.parametrize("H,W", [(16, 256), (32, 512)])
@pytest.mark.parametrize("at", ["identity", "registered"])
def test_room_parity(oracle, H, W, at):
    *sets, registered = room(oracle, H, W)
    pose = IDENT if at == "identity" else registered
    info, m = record_and_model(sets, pose, f"room {H}x{W} at {at}")
    assert m["n_edge"] > 30 and m["n_plane"] > 500 and m["n_dropped"] == 0
    if (H, W, at) == (16, 256, "registered"):  # the census of the oracle's association: 69 + 950 rows, none in the Huber region
        assert (m["n_edge"], m["n_plane"], m["n_huber"]) == (69, 950, 0)
        assert np.allclose(info.eigenvalues, [283, 304, 406, 6217, 8108, 11327], rtol=2e-3)
    # the remaining gradient says whether the pose sits at a minimum: it is smaller at the registered pose than at identity
    if at == "registered":
        at_identity = ctx().registration_information(*sets, pose=IDENT)
        assert np.linalg.norm(info.gradient) < np.linalg.norm(at_identity.gradient)


def test_huber_region(oracle):
    *sets, _ = room(oracle, 16, 256)
    info, m = record_and_model(sets, np.array([0, 0, 0, 1.0, 0, 0, 1.3]), "room 16x256, 1.3 m off")
    assert m["n_huber"] >= 100 and m["n_edge"] > 30 and m["n_plane"] > 500  # (CPU census: 49 + 909 rows, 201 beyond r^2 = 1)
    assert int(info.n_huber) == m["n_huber"]


def test_dropped_rows_of_a_scene_registered_against_itself():
    edge, planar = (np.ascontiguousarray(x, dtype=np.float64) for x in K.registration_scene())
    assert (len(edge), len(planar)) == (162, 8941)
    sets = (edge, planar, edge, planar)
    info, m = record_and_model(sets, IDENT, "KAT scene against itself")
    # every edge point is its own nearest neighbour and lies exactly on the line fitted through its neighbours: |c| = 0
    assert m["n_dropped"] == 162 and m["n_edge"] == 0 and m["n_plane"] > 5000
    assert int(info.n_dropped) == 162 and int(info.n_edge) == 0
    assert np.all(np.isfinite(I.record_sums(info))) and np.all(np.isfinite(info.eigenvalues)) and np.all(np.isfinite(info.eigenvectors))


def test_degeneracy_of_the_corridor_and_its_end_wall():
    sets = I.corridor()
    assert [len(x) for x in sets] == [196, 1568, 484, 3872]
    info, m = record_and_model(sets, IDENT, "corridor")
    assert (m["n_edge"], m["n_plane"]) == (196, 1568)
    fro = np.linalg.norm(info.information)
    print("corridor eigenvalues", info.eigenvalues, "v0", info.eigenvectors[0])
    assert abs(info.eigenvalues[0]) <= 128 * I.EPS * fro
    assert abs(info.eigenvectors[0][4]) >= 1 - 1e-9  # t_y: along the corridor
    assert info.eigenvalues[1] > 100  # (CPU: 784)
    deg = info.degenerate_directions(100.0)
    assert deg.shape == (1, 6) and abs(deg[0][4]) >= 1 - 1e-9
    sets = I.corridor(end_wall=True)
    assert [len(x) for x in sets] == [196, 1768, 484, 4272]
    info, m = record_and_model(sets, IDENT, "corridor with end wall")
    print("with end wall", info.eigenvalues)
    assert m["n_plane"] > 1568 + 100
    assert info.eigenvalues[0] > 100  # (CPU: 200)
    assert len(info.degenerate_directions(100.0)) == 0


def test_covariance_equals_the_numpy_helper(oracle):
    *sets, registered = room(oracle, 16, 256)
    info = ctx().registration_information(*sets, pose=registered)
    want = I.covariance_numpy(info.information, info.weighted_sq_error, int(info.n_edge) + int(info.n_plane))
    assert np.abs(info.covariance() - want).max() <= 1e-12 * np.abs(want).max()


def test_all_twelve_registration_fields_reach_the_information_pass(oracle):
    """a parameter set with every field off its default and pairwise distinct (tests/reg_param_scenes.py: binding_sets), the plane
    gate negative so that it acts: n_edge / n_plane are the model's, built from the association dump under the same parameters,
    and differ from the counts under the default parameters and under each association field reset alone."""
    import reg_param_scenes as S
    over = S.binding_sets(oracle)["converged"]
    sets = S.binding_room()
    c = ctx()

    def counts(fields):
        reg = S.params(capi.RegistrationParams, **fields)
        info = c.registration_information(*sets, pose=IDENT, reg=reg)
        m = I.model(*I.records_of_dump(c.associate(*sets, IDENT, reg)))
        I.check_against_model(info, m, "binding set")
        return int(info.n_edge), int(info.n_plane)

    base = counts(over)
    valid_e, _, _, _ = oracle.associate(sets[0], sets[2], IDENT, False, S.params(oracle.RegParams, **over))
    valid_p, _, _, _ = oracle.associate(sets[1], sets[3], IDENT, True, S.params(oracle.RegParams, **over))
    assert base == (int(valid_e.sum()), int(valid_p.sum())) and base[0] > 20 and 100 < base[1] < len(sets[1]) - 100
    assert counts({}) != base
    for f in ("num_edge_neighbors", "max_edge_neighbor_dist", "min_line_fit_points", "num_plane_neighbors", "max_plane_neighbor_dist",
              "min_plane_fit_points", "max_avg_point_plane_dist"):
        assert counts({**over, f: S.DEFAULTS[f]}) != base, f
    assert counts({**over, "min_line_condition_number": float("inf")}) == (0, base[1])
