"""What the CPU and the GPU test of the solve forms share (tests/test_solve_forms_hostcheck.py, tests/test_gpu_solve_forms.py): the
CPU census of a scene, computed once, and the assertions that a scene has the form it is named for."""
import numpy as np

import hostcheck_lib as Hc
import solve_scenes as S

IDENT = [0, 0, 0, 1.0, 0, 0, 0]
_cpu = {}


def cpu_census(name, **flags):
    """(scene, planar capacity of a single-pair call, hostcheck_register_forms' outcome), computed once per scene"""
    key = (name,) + tuple(sorted(flags.items()))
    if key not in _cpu:
        sc = S.scene(name)
        prm = Hc.reg_params()
        prm.min_associations = sc.min_assoc
        stride = max(len(sc.sp), len(sc.tp), 1)
        _cpu[key] = (sc, stride, Hc.register_forms(sc.se, sc.sp, sc.te, sc.tp, prm=prm, sweep_chunk=S.SWEEP_CHUNK,
                                                   sweep_threads=S.SWEEP_THREADS, tiles=S.n_tiles(stride), **flags))
    return _cpu[key]


def bound_lhs(cen, x):
    """left-hand side of the kernels' validity bound of one iteration's moments (its census) at candidate x"""
    return Hc.moments_bound(cen["s0max"], cen["v2max"], x, cen["mom_ref"] if cen["moments"] == 2 else None)[1]


def check_expectations(sc, stride, listed, tiles, lhs_ident, lhs_update, n_iter):
    """what the scene is for (solve_scenes._SPECS), from per-iteration lists of: listed records, listed records per live tile,
    the bound's left-hand side at the identity update and at the accepted update. Shared with the GPU test."""
    e = sc.expect
    assert n_iter >= e.get("min_iters", 1), (sc.name, n_iter)
    for i in range(n_iter):
        assert int(np.sum(tiles[i])) == listed[i], (sc.name, i)
        if "walk" in e:
            assert S.walk_of(stride, listed[i]) == e["walk"], (sc.name, i, listed[i])
        if "listed" in e:
            assert e["listed"][0] <= listed[i] <= e["listed"][1], (sc.name, i, listed[i])
        assert abs(listed[i] - S.FLAT_CACHE) >= 40, (sc.name, i, listed[i])  # (rounding cannot flip the walk of any scene)
        if e.get("every_tile"):
            assert len(tiles[i]) >= 4 and np.all(tiles[i] > 0), (sc.name, i, tiles[i])
        if e.get("big_and_hole"):
            t = np.asarray(tiles[i])
            assert t.max() > 64, (sc.name, i, t)
            assert any(t[k] == 0 and t[:k].any() and t[k + 1:].any() for k in range(len(t))), (sc.name, i, t)
        if e.get("calm"):
            assert lhs_update[i] <= 0.5, (sc.name, i, lhs_update[i])
    if e.get("streams"):
        assert any(lhs_update[i] >= 2.0 and lhs_ident[i] < 0.999 for i in range(1, n_iter)), (sc.name, lhs_ident, lhs_update)
