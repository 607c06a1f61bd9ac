"""GPU: surfel localisation (include/loamx.h, "surfel localisation"; loam_amd/csrc/localize_kernels.hip) against the host build of
localize_math.h (tests/hostcheck_localize, which tests/test_localize_hostcheck.py compares with an independent numpy model) BY
BYTES: the poses, the 128-byte result records and the 696-byte information records. The device map and the Python surfel model
behind the host build are filled from the same clouds (tests/test_gpu_surfel.py compares those two by bytes). Outputs are poisoned
before every call. The plane cache and the plain form (context option NO_LOCALIZE_PLANES) must agree with the host build alike.

MEASURED: the information matrix of one evaluation against sum J^T J formed in numpy from the surfel map's own query records, largest
entry-wise deviation relative to the largest entry: 5.1e-16 (lot), 4.1e-16 (canyon) -> INFO_TOL = 8 x 5.1e-16."""
import ctypes as C

import numpy as np
import pytest

import localize_common as L
import surfel_common as M
from gpu_common import ctx, option
from loam_amd import capi

pytestmark = pytest.mark.gpu

POISON = 0xA5
INFO_TOL = 8 * 5.1e-16
FORMS = [pytest.param(0, id="planes"), pytest.param(1, id="plain")]


def test_the_layers_agree_on_the_records():
    assert capi.LOCALIZE_RESULT_DTYPE == L.RESULT_DTYPE and capi.INFORMATION_DTYPE.itemsize == L.INFO_DTYPE.itemsize == 696
    p = capi.LocalizeParams()
    assert {n: getattr(p, n) for n in L.PARAM_NAMES} == L.DEFAULTS
    assert C.sizeof(capi.LocalizeParamsStruct) == L.PARAMS_DTYPE.itemsize
    assert [f[0] for f in capi.LocalizeParamsStruct._fields_] == list(L.PARAMS_DTYPE.names)
    assert (capi.LOCALIZE_CONVERGED, capi.LOCALIZE_MAX_ITERATIONS, capi.LOCALIZE_TOO_FEW_ROWS, capi.LOCALIZE_NOT_FINITE) == \
        (L.CONVERGED, L.MAX_ITERATIONS, L.TOO_FEW_ROWS, L.NOT_FINITE)


def device_map(model, max_voxels=1 << 15, c=None):
    """a device surfel map with the voxels of a model of localize_common (its recipe, through the device add)"""
    c = c or ctx()
    m = c.surfel_map(capi.SurfelMapParams(model.leaf, model.min_range, model.max_range), max_voxels)
    pts, offsets, poses = model.recipe
    bufs = [c.alloc(max(pts.nbytes, 8)).upload(np.ascontiguousarray(pts, dtype=np.float64))]
    if poses is not None:
        bufs.append(c.alloc(poses.nbytes).upload(np.ascontiguousarray(poses, dtype=np.float64)))
    m.add_clouds_dev(bufs[0].ptr, 3, offsets, bufs[1].ptr if poses is not None else 0)
    c.synchronize()
    for b in bufs:
        b.free()
    assert m.stats()["voxels"] == len(model.vox) and m.stats()["overflow"] == 0
    return m


def poisoned(c, nbytes):
    return c.alloc(nbytes).upload(np.full(nbytes, POISON, dtype=np.uint8))


def is_poison(a):
    return bool((np.ascontiguousarray(a).reshape(-1).view(np.uint8) == POISON).all())


def dev_run(loc, points, offsets, poses, p, in_place=False, info=True, expect=None):
    """run_dev on uploaded clouds into poisoned outputs with one spare record behind each; dict(poses, results, info). expect: the
    status of a refusal; then every output must still be poison (the poses: unchanged)."""
    c = loc.ctx
    pts = np.ascontiguousarray(points)
    assert pts.dtype in (np.float32, np.float64) and pts.ndim == 2
    n = len(offsets) - 1
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(n, 7)
    d_pts = c.alloc(max(pts.nbytes, 8))
    d_in = poisoned(c, (n + 1) * 56)
    d_out = d_in if in_place else poisoned(c, (n + 1) * 56)
    d_res, d_info = poisoned(c, (n + 1) * 128), poisoned(c, (n + 1) * 696)
    try:
        if pts.size:
            d_pts.upload(pts)
        if n:
            d_in.upload(poses)
        params = capi.LocalizeParams(**p) if isinstance(p, dict) else p
        try:
            loc.run_dev(d_pts.ptr, pts.shape[1], offsets, d_in.ptr, d_out.ptr, d_res.ptr, d_info.ptr if info else 0, params, f32=pts.dtype == np.float32)
            status = 0
        except capi.LoamxError as e:
            status = e.status
        c.synchronize()
        out = dict(poses=d_out.download(np.float64, (n + 1) * 7).reshape(n + 1, 7), results=d_res.download(L.RESULT_DTYPE, n + 1),
                   info=d_info.download(L.INFO_DTYPE, n + 1))
    finally:
        for b in {d_pts, d_in, d_out, d_res, d_info}:
            b.free()
    assert status == (expect or 0), (status, expect, c.lib.loamx_last_error(c.h))
    if expect:
        assert is_poison(out["results"]) and is_poison(out["info"]) and is_poison(out["poses"][n:])
        assert in_place or is_poison(out["poses"])
        assert not in_place or n == 0 or M.same_bytes(out["poses"][:n], poses)
        return None
    assert is_poison(out["poses"][n:]) and is_poison(out["results"][n:]) and is_poison(out["info"][n if info else 0:]), "written past the call's clouds"
    return dict(poses=out["poses"][:n].copy(), results=out["results"][:n].copy(), info=out["info"][:n].copy() if info else None)


def assert_same(dev, host, what=""):
    for k in ("poses", "results", "info"):
        if dev[k] is None:
            continue
        if M.same_bytes(dev[k], host[k]):
            continue
        bad = [i for i in range(len(host[k])) if not M.same_bytes(dev[k][i:i + 1], host[k][i:i + 1])]
        raise AssertionError((what, k, "clouds", bad[:8], dev[k][bad[0]], host[k][bad[0]]))


@pytest.fixture(scope="module")
def lot():
    """(model, device map, localiser, scans, poses) of the lot drive, shared: no test changes the map"""
    model = L.drive_map("lot")
    m = device_map(model)
    loc = m.localizer(max_clouds=320, max_points=1 << 16)
    scans, poses = L.drive("lot")
    yield model, m, loc, scans, poses
    loc.close()
    m.close()


def pool(scans):
    return np.concatenate([scans[6], scans[5], scans[4]])


@pytest.mark.parametrize("plain", FORMS)
def test_cloud_sizes_around_the_workgroup_and_the_chunk(lot, plain):
    model, m, loc, scans, poses = lot
    sizes = [0, 1, 255, 256, 257, L.CHUNK - 1, L.CHUNK, L.CHUNK + 1, 2 * L.CHUNK + 3]
    pts = pool(scans)
    clouds = [pts[:k] for k in sizes]  # (the last cloud runs on into a second and a third scan: it only has to give the same bytes)
    inits = np.stack([L.displaced(poses[6], 0.1, 0.5, seed=i) for i in range(len(sizes))])
    off = np.concatenate([[0], np.cumsum(sizes)])
    p = L.params(min_rows=20, max_iterations=4)
    host = L.host_run(model, np.concatenate(clouds), off, inits, p)
    assert set(host["results"]["termination"].tolist()) >= {L.TOO_FEW_ROWS, L.CONVERGED} and host["results"]["n_rows"][-1] > 2000
    before = m.emit()
    with option("NO_LOCALIZE_PLANES", plain):
        dev = dev_run(loc, np.concatenate(clouds), off, inits, p)
        assert_same(dev, host, "sizes")
        again = dev_run(loc, np.concatenate(clouds), off, inits, p)
        assert_same(again, dev, "two runs")
        for c in (2, 5, 7):  # one cloud alone against the same cloud inside the batch
            alone = dev_run(loc, clouds[c], [0, sizes[c]], inits[c][None], p)
            assert_same(alone, {k: v[c:c + 1] for k, v in dev.items()}, f"cloud {c} alone")
    M.assert_emit_equal(m.emit(), before, "the map after a run")


@pytest.mark.parametrize("plain", FORMS)
@pytest.mark.parametrize("dtype,stride", [(np.float64, 3), (np.float64, 5), (np.float32, 3), (np.float32, 5)])
def test_three_clouds_with_an_empty_one_in_the_middle_f64_f32_stride_in_place(lot, plain, dtype, stride):
    model, m, loc, scans, poses = lot
    rng = np.random.default_rng(5)
    pts = np.concatenate([scans[6], scans[5]]).astype(dtype)
    wide = rng.normal(size=(len(pts), stride)).astype(dtype)
    wide[:, :3] = pts
    off = [0, 4096, 4096, 8192]
    inits = np.stack([L.displaced(poses[6]), poses[6], L.displaced(poses[5], 0.1, 1.0, seed=9)])
    p = L.params()
    host = L.host_run(model, wide, off, inits, p)
    assert host["results"]["termination"].tolist() == [L.CONVERGED, L.TOO_FEW_ROWS, L.CONVERGED]
    with option("NO_LOCALIZE_PLANES", plain):
        assert_same(dev_run(loc, wide, off, inits, p), host, "out of place")
        assert_same(dev_run(loc, wide, off, inits, p, in_place=True, info=False), host, "in place")


@pytest.mark.parametrize("plain", FORMS)
def test_two_launch_groups(lot, plain):
    model, m, loc, scans, poses = lot
    n = L.CHUNK_CLOUDS + 44
    ground = scans[6][np.linalg.norm(scans[6], axis=1) > 1.0]
    clouds = [ground[13 * i:13 * i + 40] for i in range(n)]  # (overlapping pieces of one scan)
    assert all(len(c) == 40 for c in clouds)
    off = np.arange(n + 1) * 40
    inits = np.stack([L.displaced(poses[6], 0.03, 0.2, seed=i) for i in range(n)])
    p = L.params(min_rows=12, max_iterations=3)
    host = L.host_run(model, np.concatenate(clouds), off, inits, p)
    assert (host["results"]["iterations"][L.CHUNK_CLOUDS:] > 0).any() and len(set(host["results"]["termination"].tolist())) >= 2
    with option("NO_LOCALIZE_PLANES", plain):
        assert_same(dev_run(loc, np.concatenate(clouds), off, inits, p), host, "300 clouds")


@pytest.mark.parametrize("plain", FORMS)
def test_clouds_of_a_batch_stop_at_different_iterations(lot, plain):
    model, m, loc, scans, poses = lot
    p = L.params(max_iterations=3)
    bad = poses[6].copy()
    bad[4] = np.inf
    clouds = [scans[6], scans[6], scans[6][:120], scans[6][:0], scans[6]]
    inits = np.stack([L.displaced(poses[6], 0.02, 0.1), L.displaced(poses[6], 0.6, 4.0, seed=2), poses[6], poses[6], bad])
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    host = L.host_run(model, np.concatenate(clouds), off, inits, p)  # (asserted on the host build first)
    assert host["results"]["termination"].tolist() == [L.CONVERGED, L.MAX_ITERATIONS, L.TOO_FEW_ROWS, L.TOO_FEW_ROWS, L.NOT_FINITE]
    with option("NO_LOCALIZE_PLANES", plain):
        assert_same(dev_run(loc, np.concatenate(clouds), off, inits, p), host, "mixed batch")
    p0 = L.params(max_iterations=0)
    host = L.host_run(model, np.concatenate(clouds), off, inits, p0)
    with option("NO_LOCALIZE_PLANES", plain):
        dev = dev_run(loc, np.concatenate(clouds), off, inits, p0)
    assert_same(dev, host, "max_iterations 0")
    assert M.same_bytes(dev["poses"], inits)


@pytest.mark.parametrize("plain", FORMS)
def test_every_candidate_and_gate_case(plain):
    for name, (model, pts, pose, p, want) in sorted(L.micro_cases().items()):
        host = L.host_run(model, pts, [0, len(pts)], pose[None], p)
        m = device_map(model, 1 << 8)
        loc = m.localizer(1, 16)
        try:
            with option("NO_LOCALIZE_PLANES", plain):
                assert_same(dev_run(loc, pts, [0, len(pts)], pose[None], p), host, name)
        finally:
            loc.close()
            m.close()


def test_floor_only_map_and_the_canyon(lot):
    model, pts, truth = L.floor_map()
    p = L.params(min_eigenvalue_per_row=0.01)
    cloud, init = pts[::7], L.displaced(truth, 0.1, 1.0, seed=3)
    host = L.host_run(model, cloud, [0, len(cloud)], init[None], p)
    assert host["results"][0]["used_mask"] == 0b111000
    m = device_map(model, 1 << 13)
    loc = m.localizer(1, len(cloud))
    try:
        assert_same(dev_run(loc, cloud, [0, len(cloud)], init[None], p), host, "floor")
        pose, res, info = loc.run(cloud, init, capi.LocalizeParams(**p))  # the host form
        assert M.same_bytes(pose, host["poses"][0]) and M.same_bytes(np.array([res]), host["results"]) and M.same_bytes(np.array([info]), host["info"])
        pose32, res32, none = loc.run(cloud.astype(np.float32), init, capi.LocalizeParams(**p), information=False)
        host32 = L.host_run(model, cloud.astype(np.float32), [0, len(cloud)], init[None], p)
        assert none is None and M.same_bytes(np.array([res32]), host32["results"])
    finally:
        loc.close()
        m.close()
    cmodel = L.drive_map("canyon")
    scans, poses = L.drive("canyon")
    init = L.displaced(poses[6])
    host = L.host_run(cmodel, scans[6], [0, 4096], init[None], L.params())
    m = device_map(cmodel)
    loc = m.localizer(1, 4096)
    try:
        assert_same(dev_run(loc, scans[6], [0, 4096], init[None], L.params()), host, "canyon")
        assert host["results"][0]["termination"] == L.CONVERGED
    finally:
        loc.close()
        m.close()


def test_information_agrees_with_the_sum_formed_from_query_records(lot):
    model, m, loc, scans, poses = lot
    p = L.params(neighborhood=1, max_iterations=0)
    init = L.displaced(poses[6])
    dev = dev_run(loc, scans[6], [0, 4096], init[None], p)
    ok = L.CM.validity(scans[6], model.min_range, model.max_range) == L.CM.USED
    v = L.CM.pose_act(init, scans[6][ok])
    rec, dist, cnt = m.query(v, min_points=p["min_points"])
    H, n = L.information_from_records(rec, dist, v, p, model.leaf)
    dev_h = dev["info"][0]["information"]
    deviation = np.abs(H - dev_h).max() / np.abs(H).max()
    print(f"information against query records: {n} rows, deviation {deviation:.3g}")
    assert n == dev["results"][0]["n_rows"] > 1000
    assert deviation <= INFO_TOL, deviation


def test_refusals_leave_the_outputs_untouched(lot):
    model, m, loc, scans, poses = lot
    pts, off, init = scans[6], [0, 4096], poses[6][None]
    BAD, UNS = capi.ERR_BAD_PARAM, capi.ERR_UNSUPPORTED
    for kw in (dict(neighborhood=3), dict(neighborhood=0), dict(planarity=-0.1), dict(planarity=np.nan), dict(max_distance=-1.0),
               dict(max_distance=np.inf), dict(huber_delta=-0.1), dict(rotation_convergence_thresh=np.nan),
               dict(position_convergence_thresh=-1.0), dict(min_eigenvalue_per_row=np.inf)):
        dev_run(loc, pts, off, init, L.params(**kw), expect=BAD)
        dev_run(loc, pts, off, init, L.params(**kw), expect=BAD, in_place=True)
    dev_run(loc, pts, off, init, L.params(max_iterations=1001), expect=UNS)
    dev_run(loc, pts, [0, 4096, 4000], np.stack([poses[6]] * 2), L.params(), expect=BAD)  # decreasing offsets
    dev_run(loc, np.zeros((8, 2)), [0, 8], init, L.params(), expect=BAD)  # point_stride < 3
    small = m.localizer(2, 100)
    try:
        dev_run(small, pts, [0, 10, 20, 30], np.stack([poses[6]] * 3), L.params(), expect=UNS)  # n_clouds > max_clouds
        dev_run(small, pts, [0, 101], init, L.params(), expect=UNS)  # more points than max_points
        assert dev_run(small, pts, [0, 100], init, L.params())["results"][0]["termination"] in (L.CONVERGED, L.TOO_FEW_ROWS, L.MAX_ITERATIONS)
    finally:
        small.close()
    c = loc.ctx
    st = capi.LocalizeParams().struct()
    o = np.array([0, 16], dtype=np.uint64)
    szp = o.ctypes.data_as(C.POINTER(C.c_size_t))
    d = poisoned(c, 4096)
    try:
        run = c.lib.loamx_surfel_localizer_run
        assert run(c.h, None, d.ptr, 3, szp, 1, d.ptr, d.ptr, d.ptr, None, C.byref(st)) == BAD
        assert run(c.h, loc._handle(), d.ptr, 3, szp, 1, None, d.ptr, d.ptr, None, C.byref(st)) == BAD
        assert run(c.h, loc._handle(), d.ptr, 3, szp, 1, d.ptr, None, d.ptr, None, C.byref(st)) == BAD
        assert run(c.h, loc._handle(), d.ptr, 3, szp, 1, d.ptr, d.ptr, None, None, C.byref(st)) == BAD
        assert run(c.h, loc._handle(), None, 3, szp, 1, d.ptr, d.ptr, d.ptr, None, C.byref(st)) == BAD
        assert run(c.h, loc._handle(), d.ptr, 3, None, 1, d.ptr, d.ptr, d.ptr, None, C.byref(st)) == BAD
        assert run(c.h, loc._handle(), d.ptr, 3, szp, 1, d.ptr, d.ptr, d.ptr, None, None) == BAD
        assert run(c.h, loc._handle(), d.ptr, 3, szp, 0, None, None, None, None, C.byref(st)) == capi.OK  # no clouds: nothing to do
        h = C.c_void_p()
        assert c.lib.loamx_surfel_localizer_create(c.h, None, 1, 1, C.byref(h)) == BAD
        assert c.lib.loamx_surfel_localizer_create(c.h, m._handle(), 0, 1, C.byref(h)) == BAD
        assert c.lib.loamx_surfel_localizer_create(c.h, m._handle(), 1, 1, None) == BAD
        assert c.lib.loamx_surfel_localizer_create(c.h, m._handle(), (1 << 24) + 1, 1, C.byref(h)) == UNS
        c.synchronize()
        assert is_poison(d.download(np.uint8, 4096))
    finally:
        d.free()
    with pytest.raises(ValueError):
        loc.run(np.zeros((4, 2)), poses[6])
    with pytest.raises(ValueError):
        loc.run(scans[6], poses[6][:6])
    with pytest.raises(ValueError):
        capi.LocalizeParams(leaf=1.0)
    with pytest.raises(ValueError):
        m.localizer(-1, 10)


def test_a_second_context_is_refused(lot):
    model, m, loc, scans, poses = lot
    other = capi.Context(0)
    try:
        h = C.c_void_p()
        assert other.lib.loamx_surfel_localizer_create(other.h, m._handle(), 1, 16, C.byref(h)) == capi.ERR_BAD_PARAM and not h.value
        st = capi.LocalizeParams().struct()
        o = np.array([0, 16], dtype=np.uint64)
        d = other.alloc(4096).upload(np.full(4096, POISON, dtype=np.uint8))
        rc = other.lib.loamx_surfel_localizer_run(other.h, loc._handle(), d.ptr, 3, o.ctypes.data_as(C.POINTER(C.c_size_t)), 1, d.ptr, d.ptr, d.ptr,
                                                  None, C.byref(st))
        other.synchronize()
        assert rc == capi.ERR_BAD_PARAM and is_poison(d.download(np.uint8, 4096))
        d.free()
    finally:
        other.close()


def test_a_drive_without_a_synchronise_equals_the_host_forms():
    """The hand-over the localiser was built for, on the 16 x 256 lot drive, with nothing waiting on the host before the emit:
    organise seven shuffled clouds into scans -> compose the trajectory on the device from the relative motions (the true ones for
    the first four scans, odometry 0.04 m / 0.2 degrees off per step for the rest) -> add the first four scans at their composed
    poses -> per further scan: localise the ORGANISED scan (empty cells and all) in place from its composed pose, a device array the
    trajectory kernel wrote in the same stream, and add it at the localised pose -> emit. The same chain in the host forms
    (organize_cloud, add_cloud, run; the trajectory has no host form: it is composed by the same entry point, synchronised and
    downloaded) gives the same bytes: the scans, the poses, the result records and the emitted map."""
    import organize_common as OC
    import outdoor_scenes as S
    scans, poses = L.drive("lot")
    c = ctx()
    n0, n, per = 4, 7, L.H * L.W
    rng = np.random.default_rng(61)
    clouds = np.ascontiguousarray(np.stack([scans[i][rng.permutation(per)] for i in range(n)]))
    rel = [L.compose(L.inverse(poses[i]), poses[i + 1]) for i in range(n - 1)]
    for i in range(n0 - 1, n - 1):
        rel[i] = L.displaced(rel[i], 0.04, 0.2, seed=i)
    results = np.zeros(n - 1, dtype=capi.RESULT_DTYPE)
    results["pose"] = np.stack(rel)
    p = capi.LocalizeParams()
    lay = c.scan_layout(capi.LidarParams(L.H, L.W, 1.0, 120.0), capi.OrganizeParams(elevations=OC.fan_elevations(L.H, S.FANS["lot"])))
    maps = [c.surfel_map(capi.SurfelMapParams(0.5, 0.5, 120.0), 1 << 15) for _ in range(2)]
    locs = [mm.localizer(1, per) for mm in maps]
    d_clouds, d_scans = c.alloc(clouds.nbytes).upload(clouds), poisoned(c, clouds.nbytes)
    d_results, d_traj, d_res = c.alloc(results.nbytes).upload(results), poisoned(c, n * 56), poisoned(c, 128 * n)
    try:
        each = per * 24
        c.synchronize()
        c.organize_clouds_dev(lay, d_clouds.ptr, 3, np.arange(n + 1) * per, d_scans.ptr)
        c.compose_trajectory_dev(d_results.ptr, n - 1, d_traj.ptr, origin=poses[0])
        maps[0].add_clouds_dev(d_scans.ptr, 3, np.arange(n0 + 1) * per, d_traj.ptr)
        for i in range(n0, n):
            locs[0].run_dev(d_scans.ptr + i * each, 3, [0, per], d_traj.ptr + 56 * i, d_traj.ptr + 56 * i, d_res.ptr + 128 * i, 0, p)
            maps[0].add_clouds_dev(d_scans.ptr + i * each, 3, [0, per], d_traj.ptr + 56 * i)
        got = maps[0].emit()  # (the first wait on the host)
        got_scans = d_scans.download(np.float64, n * per * 3).reshape(n, per, 3)
        got_traj, got_res = d_traj.download(np.float64, n * 7).reshape(n, 7), d_res.download(L.RESULT_DTYPE, n)
        assert is_poison(got_res[:n0])
        # what the organiser left is not the scan as it was cast: cells without a point are in it (and must pass through validity)
        empty = ~np.isfinite(got_scans).all(axis=2) | ~got_scans.any(axis=2)
        assert empty[n0:].any(axis=1).all() and (~empty[n0:]).sum(axis=1).min() > 3000, empty.sum(axis=1)

        # the host forms
        c.compose_trajectory_dev(d_results.ptr, n - 1, d_traj.ptr, origin=poses[0])
        c.synchronize()
        odo = d_traj.download(np.float64, n * 7).reshape(n, 7)
        assert M.same_bytes(odo[:n0], got_traj[:n0]) and not M.same_bytes(odo[n0:], got_traj[n0:])
        for i in range(n0, n):  # the odometry is off by what was put into it, the true part of the trajectory by rounding only
            before = L.pose_error(odo[i], poses[i])
            assert 0.03 < before[0] < 0.2 and L.pose_error(odo[n0 - 1], poses[n0 - 1])[0] < 1e-9, (i, before)
        host_scans = [c.organize_cloud(clouds[i], lay)[0] for i in range(n)]
        assert M.same_bytes(np.stack(host_scans), got_scans)
        for i in range(n0):
            maps[1].add_cloud(host_scans[i], odo[i])
        want_res = []
        for i in range(n0, n):
            pose, r, _ = locs[1].run(host_scans[i], odo[i], p, information=False)
            want_res.append(r)
            maps[1].add_cloud(host_scans[i], pose)
            assert M.same_bytes(pose, got_traj[i]), i
            after, before = L.pose_error(pose, poses[i]), L.pose_error(odo[i], poses[i])
            assert after[0] < before[0] and after[1] < before[1], (i, before, after)  # nearer the truth than the odometry, in both
        M.assert_emit_equal(got, maps[1].emit(), "the chain")
        assert M.same_bytes(got_res[n0:], np.array(want_res)) and (got_res[n0:]["termination"] == L.CONVERGED).all()
        assert (got_res[n0:]["n_unused"] >= empty[n0:].sum(axis=1)).all()  # the empty cells were counted, not used
    finally:
        for o in locs + maps + [lay]:
            o.close()
        for b in (d_clouds, d_scans, d_results, d_traj, d_res):
            b.free()
