"""CPU-only: raycast_math.h — validity, the walk with its entry and exit parameters, the test of a voxel, the step cap, the record
and the rendered return of the ray cast kernels (loam_amd/csrc/raycast_kernels.hip) — compiled with g++ (tests/hostcheck_raycast)
against the Python model of tests/raycast_common.py, by equality, t_enter and t_exit as bit patterns. The GPU tests
(test_gpu_raycast.py) compare the kernels with the same model."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import occupancy_common as OM
import raycast_common as M

dp, u64p, u32p = C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)


def _table(vox):
    keys = np.array(sorted(vox), dtype=np.uint64)
    words = np.array([(vox[int(k)][0] << 32) | vox[int(k)][1] for k in keys], dtype=np.uint64)
    return keys, words


def _params(P):
    P = dict(M.DEFAULTS, **P)
    return np.array([P["skip_start"], P["unknown_stops"], P["max_steps"], P["hit_at"]], dtype=np.uint32)


def header_cast(origins, ends, leaf, vox, rule, P):
    o, e = np.ascontiguousarray(origins, dtype=np.float64), np.ascontiguousarray(ends, dtype=np.float64)
    keys, words = _table(vox)
    par = _params(P)
    out = np.zeros(len(o), dtype=M.RECORD_DTYPE)
    M.hostcheck_lib().hostcheck_raycast_cast(o.ctypes.data_as(dp), e.ctypes.data_as(dp), C.c_uint64(len(o)), C.c_double(leaf), keys.ctypes.data_as(u64p),
                                             words.ctypes.data_as(u64p), C.c_uint64(len(keys)), C.c_uint32(rule[0]), C.c_double(rule[1]),
                                             C.c_uint32(rule[2]), par.ctypes.data_as(u32p), out.ctypes.data_as(C.c_void_p))
    return out


def header_render(dirs, poses, max_range, leaf, vox, rule, P):
    d, p = np.ascontiguousarray(dirs, dtype=np.float64), np.ascontiguousarray(poses, dtype=np.float64)
    keys, words = _table(vox)
    par = _params(P)
    n = len(d) * len(p)
    scans, ranges, out = np.full((len(p), len(d), 3), 7.0), np.full((len(p), len(d)), 7.0), np.zeros((len(p), len(d)), dtype=M.RECORD_DTYPE)
    M.hostcheck_lib().hostcheck_raycast_render(d.ctypes.data_as(dp), C.c_uint64(len(d)), p.ctypes.data_as(dp), C.c_uint64(len(p)), C.c_double(max_range),
                                               C.c_double(leaf), keys.ctypes.data_as(u64p), words.ctypes.data_as(u64p), C.c_uint64(len(keys)),
                                               C.c_uint32(rule[0]), C.c_double(rule[1]), C.c_uint32(rule[2]), par.ctypes.data_as(u32p),
                                               scans.ctypes.data_as(dp), ranges.ctypes.data_as(dp), out.ctypes.data_as(C.c_void_p))
    assert n == out.size
    return scans, ranges, out


def header_visits(o, e, leaf):
    lib = M.hostcheck_lib()
    lib.hostcheck_raycast_visits.restype = C.c_uint32
    o, e = np.array(o, dtype=np.float64), np.array(e, dtype=np.float64)
    n = lib.hostcheck_raycast_visits(o.ctypes.data_as(dp), e.ctypes.data_as(dp), C.c_double(leaf), C.c_uint32(0), None, None, None)
    keys, t0, t1 = np.zeros(n, dtype=np.uint64), np.zeros(n), np.zeros(n)
    assert lib.hostcheck_raycast_visits(o.ctypes.data_as(dp), e.ctypes.data_as(dp), C.c_double(leaf), C.c_uint32(n), keys.ctypes.data_as(u64p),
                                        t0.ctypes.data_as(dp), t1.ctypes.data_as(dp)) == n
    return keys, t0, t1


HAND = M.hand_model()
CASES = M.ray_cases()
RULE = (1, 0.0, 1)


@pytest.mark.parametrize("variant", sorted(M.PARAM_VARIANTS))
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_model_equals_the_g_plus_plus_build_on_the_cases_of_the_rule(name, variant):
    o, e = CASES[name]
    P = M.PARAM_VARIANTS[variant]
    want, _ = M.cast(o, e, M.LEAF, M.StateMap.of(HAND), P)
    got = header_cast(o, e, M.LEAF, HAND.vox, RULE, P)
    assert M.same_bytes(got, want), (name, variant, got, want)


def test_what_the_cases_are_there_for_is_what_the_model_says_of_them():
    """A check of the REFERENCE only: the model's records on the hand-made map against statuses worked out by hand."""
    states = M.StateMap.of(HAND)
    run = lambda name, **P: M.cast(*CASES[name], M.LEAF, states, P)[0]
    assert run("o_equals_e")["status"].tolist() == [M.CLEAR, M.HIT, M.CLEAR] and run("o_equals_e")["visits"].tolist() == [1, 1, 1]
    assert run("o_equals_e")["n_unknown"].tolist() == [0, 0, 1] and run("o_equals_e", unknown_stops=1)["status"].tolist() == [M.CLEAR, M.HIT, M.UNKNOWN]
    r = run("along_an_axis")
    assert r["status"].tolist() == [M.HIT, M.HIT] + [M.CLEAR] * 4 and r["voxel"][:2].tolist() == [[8, 0, 0], [-6, 0, 0]]
    assert r["visits"].tolist() == [9, 7, 13, 13, 13, 13] and (r["n_unknown"][2:] > 0).all()
    r = run("lattice_corner_diagonals")  # exact ties on three axes: x first, then y, then z
    tr = []
    M.cast_one([0.0, 0.0, 0.0], [3.0, 3.0, 3.0], M.LEAF, states, dict(M.DEFAULTS), tr)
    assert np.diff(OM.key_coords([t[0] for t in tr[:4]]), axis=0).tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    assert [t[2] for t in tr[:4]] == [0.0, tr[0][3], tr[0][3], tr[0][3]]  # the three tied steps enter at the same parameter
    r0, r1 = run("hit_in_visit_0"), run("hit_in_visit_0", skip_start=1)
    assert r0["status"].tolist() == [M.HIT, M.HIT] and r0["visits"].tolist() == [1, 1] and r0["t_enter"].tolist() == [0.0, 0.0]
    assert r1["status"].tolist() == [M.CLEAR, M.CLEAR] and (r1["visits"] > 1).all()
    r = run("hit_in_the_last_voxel")
    assert r["status"].tolist() == [M.HIT, M.HIT] and r["t_exit"].tolist() == [1.0, 1.0] and r["voxel"][:, 0].tolist() == [8, 8]
    assert run("one_voxel_short_of_the_wall")["status"].tolist() == [M.CLEAR, M.CLEAR]
    r0, r1 = run("through_a_gap_nobody_saw"), run("through_a_gap_nobody_saw", unknown_stops=1)
    assert r0["status"].tolist() == [M.HIT, M.CLEAR, M.HIT] and r0["n_unknown"][0] == 4 and r0["n_unknown"][1] > 0
    assert r1["status"].tolist() == [M.UNKNOWN] * 3 and r1["visits"][0] == 1
    n = M.STEPS_OF_THE_CAPPED_RAY
    for cap, status, visits in ((0, M.TRUNCATED, 1), (n, M.CLEAR, n + 1), (n - 1, M.TRUNCATED, n)):
        r = run("the_capped_ray", max_steps=cap)
        assert (int(r["status"][0]), int(r["visits"][0])) == (status, visits), cap
    assert run("beyond_the_voxel_range")["status"].tolist() == [M.OUTSIDE] * 3 and run("not_finite")["status"].tolist() == [M.INVALID] * 4
    assert M.same_bytes(run("not_finite"), np.array([(M.INVALID, 0, (0, 0, 0), 0, 0.0, 0.0)] * 4, dtype=M.RECORD_DTYPE))
    # the census of the run cases: one run of 64 lanes makes one look-up per trip, ABAB none fewer than the plain form, and a
    # finished lane between two lanes in the same voxel keeps them apart
    _, c = M.cast(*CASES["one_run"], M.LEAF, states)
    assert c["probes"] == (64 * (n + 1), n + 1) and c["visits"] == 64 * (n + 1)
    _, c = M.cast(*CASES["alternating_abab"], M.LEAF, states)
    assert c["probes"][0] == c["probes"][1] == c["visits"]
    _, c = M.cast(*CASES["short_even_lanes"], M.LEAF, states)
    assert c["probes"] == (32 * 2 + 32 * 8, 2 + 32 * 6)


def test_t_exit_of_a_visit_is_t_enter_of_the_next_as_the_same_double():
    rng = np.random.default_rng(2)
    for o, e in zip(rng.uniform(-8, 8, (40, 3)).tolist() + [[0.0, 0.0, 0.0]], rng.uniform(-8, 8, (40, 3)).tolist() + [[3.0, 3.0, 3.0]]):
        keys, t0, t1 = header_visits(o, e, 0.3)
        tr = []
        M.cast_one(o, e, 0.3, lambda k: OM.FREE, dict(M.DEFAULTS), tr)
        assert keys.tolist() == [t[0] for t in tr]
        assert M.same_bytes(t0, np.array([t[2] for t in tr])) and M.same_bytes(t1, np.array([t[3] for t in tr]))
        assert M.same_bytes(t1[:-1], t0[1:]) and t0[0] == 0.0 and t1[-1] == 1.0 and (np.diff(t0) >= 0).all()


def test_the_model_equals_the_g_plus_plus_build_on_3000_random_segments():
    vox, o, e = M.random_segments()
    assert len(o) == 3000
    seen = set()
    for rule, P in (((1, 0.0, 1), {}), ((2, 0.5, 2), dict(unknown_stops=1)), ((1, 0.0, 1), dict(skip_start=2, max_steps=17)), ((1, 0.75, 1), dict(max_steps=M.MAX_STEPS_LIMIT))):
        want, census = M.cast(o, e, M.LEAF, M.StateMap(vox, *rule), P)
        got = header_cast(o, e, M.LEAF, vox, rule, P)
        assert M.same_bytes(got, want), (rule, P)
        assert got["t_enter"].view(np.uint64).tolist() == want["t_enter"].view(np.uint64).tolist()
        assert got["t_exit"].view(np.uint64).tolist() == want["t_exit"].view(np.uint64).tolist()
        seen |= set(want["status"].tolist())
    assert seen >= {M.CLEAR, M.HIT, M.UNKNOWN, M.TRUNCATED}


def test_the_model_equals_the_g_plus_plus_build_on_rendered_scans():
    model, _, pose = M.room_model()
    rng = np.random.default_rng(8)
    dirs = rng.normal(size=(70, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    poses = np.stack([pose, np.concatenate([q, [0.4, 0.3, -0.2]]), np.array([0.0, 0.0, np.nan, 1.0, 0.0, 0.0, 0.0])])
    rule = (model.p["min_hits"], model.p["occ_ratio"], model.p["min_passes"])
    for hit_at in (M.AT_ENTER, M.AT_MIDDLE):
        P = dict(hit_at=hit_at)
        want = M.render(dirs, poses, 9.0, model.p["leaf"], M.StateMap.of(model), P)
        got = header_render(dirs, poses, 9.0, model.p["leaf"], model.vox, rule, P)
        for g, w, what in zip(got, want, ("scans", "ranges", "records")):
            assert M.same_bytes(g, w), (hit_at, what)
        assert (want[2]["status"][:2] == M.HIT).mean() > 0.9 and (want[2]["status"][2] == M.INVALID).all()
        assert not want[0][2].any() and not np.signbit(want[0][2]).any() and (want[1][:2][want[2]["status"][:2] == M.HIT] > 0).all()


def test_the_same_functions_are_clean_under_asan_and_ubsan_in_a_stand_alone_program():
    subprocess.check_call(["make", "-s", "-C", M.HOSTCHECK_DIR, "san"])
    out = subprocess.run([os.path.join(M.HOSTCHECK_DIR, "hostcheck_raycast_san")], capture_output=True, text=True, timeout=300)
    text = out.stdout + out.stderr
    assert out.returncode == 0 and "hostcheck_raycast ok" in out.stdout, text[-3000:]
    assert "runtime error" not in text and "AddressSanitizer" not in text, text[-3000:]
