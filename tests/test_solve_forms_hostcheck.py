"""CPU-only: the scenes of tests/solve_scenes.py have the solve forms they are named for, and the host restatement of the
kernels' launch sequence (hostcheck_register_forms: first ICF iteration = one evaluation, then moments at the first candidate)
agrees with the oracle on them. The census taken here — listed plane records per ICF iteration and per moment tile, evaluations
streamed — is what tests/test_gpu_solve_forms.py requires the library's readout to report on the GPU."""
import os
import re

import numpy as np
import pytest

import hostcheck_lib as Hc
import solve_scenes as S
from gpu_common import pose_diff
from solve_forms_common import IDENT, bound_lhs, check_expectations, cpu_census

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scene_constants_are_the_kernels():
    """solve_scenes restates five constants of loamx_internal.h (it has to place its scenes around them)"""
    text = open(os.path.join(ROOT, "loam_amd", "csrc", "loamx_internal.h")).read()
    val = lambda pat: int(re.search(pat, text).group(1))
    assert val(r"constexpr int kSweepThreads = (\d+);") == S.SWEEP_THREADS
    assert "constexpr int kSweepChunk = kSweepThreads * kSweepItems;" in text
    assert val(r"#define LOAMX_SWEEP_ITEMS (\d+)") * S.SWEEP_THREADS == S.SWEEP_CHUNK
    assert val(r"constexpr uint32_t kEdgeCache = (\d+);") == S.EDGE_CACHE
    assert val(r"constexpr uint32_t kListCache = (\d+);") == S.LIST_CACHE
    assert val(r"constexpr uint32_t kFlatCache = (\d+);") == S.FLAT_CACHE
    math = open(os.path.join(ROOT, "loam_amd", "csrc", "reg_math.h")).read()
    assert float(re.search(r"constexpr double kMomInlier = ([0-9.]+);", math).group(1)) == S.MOM_INLIER
    assert S.n_tiles(S.BIG_STRIDE) > S.LIST_CACHE >= S.n_tiles(S.BIG_STRIDE - 1)
    assert [len(S.scene("se_%d" % n).se) for n in S.SE_COUNTS] == list(S.SE_COUNTS)
    assert [len(S.scene("sp_%d" % n).sp) for n in S.SP_COUNTS] == list(S.SP_COUNTS)
    sc = S.scene("changeover")
    assert len(sc.se) == S.EDGE_CACHE and len(sc.se) < S.SWEEP_CHUNK < len(sc.se) + len(sc.sp)


@pytest.mark.parametrize("name", S.NAMES + S.EXTRA_NAMES)
def test_forms_driver_against_the_oracle_and_the_census_of_every_scene(oracle, name):
    sc, stride, (pose, term, iters, info, cen) = cpu_census(name)
    oreg = oracle.RegParams()
    oreg.min_associations = sc.min_assoc
    po, to, io, oinfo = oracle.register_features(sc.se, sc.sp, sc.te, sc.tp, None, oreg, want_info=True)
    assert (term, iters) == (to, io)
    for i in range(iters):
        assert (info[i].n_edge_associations, info[i].n_plane_associations) == (oinfo[i].n_edge_assoc, oinfo[i].n_plane_assoc), (name, i)
        rot, trans = pose_diff(oracle, np.array(list(oinfo[i].update)), np.array(list(info[i].estimate_update)))
        assert rot < 1e-7 and trans < 1e-7, (name, i, rot, trans)
    rot, trans = pose_diff(oracle, po, pose)
    assert rot < 1e-5 and trans < 1e-5, (name, rot, trans)
    if name in S.EXTRA_NAMES:
        assert (term, iters) == ((oracle.INSUFFICIENT_ASSOCIATIONS, 0) if name == "too_few" else (oracle.CONVERGED, 1))
        return
    # ---- the census: the scene has its form, far enough from the listing threshold that the GPU must count the same records
    live = S.live_tiles(stride, len(sc.sp))
    for i, c in enumerate(cen):
        assert c["moments"] == (2 if i == 0 else 1), (name, i)  # first iteration: moments at its first candidate
        assert c["min_margin"] > 1e-6, (name, i, c["min_margin"])
        assert c["evals"] <= 5 and c["evals_streamed"] >= (1 if i == 0 else 0)
        assert not c["tile_counts"][live:].any()
    upd = [np.array(list(info[i].estimate_update)) for i in range(iters)]
    lhs_i, lhs_u = [bound_lhs(c, IDENT) for c in cen], [bound_lhs(c, u) for c, u in zip(cen, upd)]
    check_expectations(sc, stride, [c["listed"] for c in cen], [c["tile_counts"][:live] for c in cen], lhs_i, lhs_u, iters)
    if sc.expect.get("streams"):  # ... and the driver did stream there
        assert any(cen[i]["evals_streamed"] > 0 and lhs_i[i] < 0.999 for i in range(1, iters)), [c["evals_streamed"] for c in cen]
    if sc.expect.get("calm"):
        assert all(c["evals_streamed"] == (1 if i == 0 else 0) for i, c in enumerate(cen))
    # ---- the capacity decides the walk where the count does not: the same lists behind more than LIST_CACHE tiles
    if name in S.TILES_NAMES:
        assert all(S.walk_of(S.BIG_STRIDE, c["listed"]) == "tiles" and S.walk_of(S.BIG_STRIDE - 1, c["listed"]) != "tiles" for c in cen)


@pytest.mark.parametrize("name", S.NAMES)
def test_forms_driver_and_the_streaming_driver_tell_the_same_story(name):
    """hostcheck_register (every evaluation of the first ICF iteration streamed: what current tests pin) and the kernels' own
    sequence differ in the order a pair's plane terms are summed, no more: terminations and iteration counts equal, poses
    within 1e-9 (the bar between the library's own routes, tests/test_gpu_multi.py), as do the NO_MOMENTS / NO_REF_MOMENTS forms"""
    sc, _, (pose, term, iters, info, cen) = cpu_census(name)
    prm = Hc.reg_params()
    prm.min_associations = sc.min_assoc
    p0, t0, i0 = Hc.register(sc.se, sc.sp, sc.te, sc.tp, prm=prm)
    assert (t0, i0) == (term, iters)
    assert np.abs(p0 - pose).max() < 1e-9, (name, np.abs(p0 - pose).max())
    for flags in (dict(no_moments=True), dict(no_ref_moments=True)):
        _, _, (p1, t1, i1, _, c1) = cpu_census(name, **flags)
        assert (t1, i1) == (term, iters), (name, flags)
        assert np.abs(p1 - pose).max() < 1e-9, (name, flags, np.abs(p1 - pose).max())
        assert c1[0]["moments"] == 0 and c1[0]["evals_streamed"] == c1[0]["evals"]
        assert all(c["moments"] == (0 if "no_moments" in flags else 1) for c in c1[1:])


def test_the_exported_bounds_are_the_header_functions():
    """hostcheck_moments_bound: the verdict is the header function's, the left-hand side found from it by bisection puts the
    verdict on the right side of 0.999 and grows by what is added to s0max"""
    rng = np.random.default_rng(5)
    for _ in range(200):
        x = np.concatenate([rng.normal(size=3) * 0.02, [1.0], rng.normal(size=3) * 0.2])
        r = np.concatenate([rng.normal(size=3) * 0.02, [1.0], rng.normal(size=3) * 0.2]) if rng.random() < 0.5 else None
        s0, v2 = rng.uniform(0, 0.5), rng.uniform(0, 60.0) ** 2
        ok, lhs = Hc.moments_bound(s0, v2, x, r)
        assert ok == (lhs < 0.999), (s0, v2, x, r, lhs)
        ok2, lhs2 = Hc.moments_bound(s0 + 0.25, v2, x, r)
        assert abs(lhs2 - lhs - 0.25) < 1e-9
    assert Hc.moments_bound(0.3, 100.0, IDENT) == (True, pytest.approx(0.3, abs=1e-12))
    assert Hc.moments_bound(0.3, 100.0, IDENT[:4] + [0.5, 0, 0], IDENT)[1] == pytest.approx(0.8, abs=1e-12)
