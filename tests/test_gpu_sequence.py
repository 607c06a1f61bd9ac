"""GPU: the scan-sequence entry points (loamx_register_scan_sequence[_dev][_f32], loamx_compose_trajectory_dev) on two
short drives through the outdoor scenes. Bars as everywhere in the suite (tests/test_gpu_outdoor.py): termination and
iteration count identical to the oracle's, SE(3) within 1e-5; against the pair entry points and between the host and
device forms the records are compared byte for byte."""
import contextlib

import numpy as np
import pytest

import outdoor_scenes as S
import sequence_common as Q
from gpu_common import ctx, option, pose_diff
from loam_amd import capi
from test_gpu_outdoor import check_record

pytestmark = pytest.mark.gpu

SE3_TOL = 1e-5
IDENT = np.array([0, 0, 0, 1.0, 0, 0, 0])


@pytest.mark.parametrize("name,n", Q.SEQUENCES)
def test_sequence_against_the_oracle(oracle, name, n):
    """every consecutive pair: the oracle extracts both scans and registers them; termination, iterations, SE(3)"""
    want = Q.oracle_pairs(oracle, name, n)
    for p, reg in enumerate(want):
        assert reg[1] != capi.INSUFFICIENT_ASSOCIATIONS, (name, p)  # (no pair of these tests is a degenerate early exit)
    res = Q.sequence_dev(ctx(), Q.sequence(name, n))
    assert len(res) == n - 1
    for p in range(n - 1):
        print(name, p, "oracle", want[p][1], want[p][2], "gpu", int(res[p]["termination"]), int(res[p]["iterations"]), pose_diff(oracle, want[p][0], res[p]["pose"]))
        check_record(oracle, res[p], want[p], (name, p))


@pytest.mark.parametrize("opt", [None, "NO_EXTRACT_BOXES"])
@pytest.mark.parametrize("name,n", Q.SEQUENCES)
def test_sequence_equals_the_pair_path_bit_for_bit(oracle, name, n, opt):
    """the sequence's records == loamx_register_scan_pairs_dev on the duplicated layout [(scan p, scan p + 1)], byte for byte:
    FP64 and float scans (those also against the oracle on the widened scans), and the sequence driven backwards"""
    c = ctx()
    scans = Q.sequence(name, n)
    with option(opt) if opt else contextlib.nullcontext():
        seq = Q.sequence_dev(c, scans)
        assert Q.same_bytes(seq, Q.pairs_dev(c, Q.duplicated(scans))), (name, opt)
        s32 = np.ascontiguousarray(scans.astype(np.float32))
        seq32 = Q.sequence_dev(c, s32)
        assert Q.same_bytes(seq32, Q.pairs_dev(c, Q.duplicated(s32))), (name, opt, "f32")
        rev = np.ascontiguousarray(scans[::-1])
        assert Q.same_bytes(Q.sequence_dev(c, rev), Q.pairs_dev(c, Q.duplicated(rev))), (name, opt, "reversed")
    want32 = Q.oracle_pairs(oracle, name, n, f32=True)
    for p in range(n - 1):
        check_record(oracle, seq32[p], want32[p], (name, p, "f32", opt))


@pytest.mark.parametrize("f32", [False, True])
def test_host_form_equals_device_form(f32):
    """loamx_register_scan_sequence (host in, host out) == the _dev records byte for byte, in one chunk (the default, 128
    pairs) and with STREAM_CHUNK_PAIRS = 3: canyon-9's 8 pairs then travel as chunks of 3, 3 and 2 pairs (4, 4 and 3 scans),
    both staging buffers are reused and there is a short tail. n_scans of 0, 1 and 2."""
    c = ctx()
    name, n = Q.SEQUENCES[0]
    scans = Q.sequence(name, n)
    if f32:
        scans = np.ascontiguousarray(scans.astype(np.float32))
    dev = Q.sequence_dev(c, scans)
    for chunk in (0, 3):
        with option("STREAM_CHUNK_PAIRS", chunk):
            got = c.register_scan_sequence(scans, n, Q.lidar())
        assert Q.same_bytes(got, dev), (chunk, f32)
    with option("STREAM_CHUNK_PAIRS", 3):
        assert Q.same_bytes(c.register_scan_sequence(scans, 5, Q.lidar()), dev[:4])  # (chunks of 3 and 1)
    # short sequences: nothing to register below two scans
    for k in (0, 1):
        assert len(c.register_scan_sequence(scans, k, Q.lidar())) == 0
        sentinel = np.full(64, 0xA5, dtype=np.uint8)
        d_xyz, d_res = c.alloc(scans[:1].nbytes).upload(scans[:1]), c.alloc(64).upload(sentinel)
        c.register_scan_sequence_dev(d_xyz.ptr, k, Q.lidar(), capi.FeatureExtractionParams(), capi.RegistrationParams(), d_res.ptr, f32=f32)
        c.synchronize()
        assert np.array_equal(d_res.download(np.uint8, 64), sentinel)
        d_xyz.free(), d_res.free()
    two = c.register_scan_sequence(scans, 2, Q.lidar())
    assert Q.same_bytes(two, Q.sequence_dev(c, scans[:2])) and Q.same_bytes(two, dev[:1])


@pytest.mark.parametrize("name,n", Q.SEQUENCES)
def test_initial_poses(oracle, name, n):
    """init[p] = the oracle's pose of pair p moved by a 0.5 degree yaw and (0.1, 0.05, 0) m: against the oracle started from
    the same pose, and byte for byte against loamx_register_features_batch_dev fed loamx_extract_features_batch_dev's output
    of the same scans with the same d_init; host form included"""
    c = ctx()
    scans = Q.sequence(name, n)
    feats, base = Q.oracle_features(oracle, name, n), Q.oracle_pairs(oracle, name, n)
    bump = S.yaw_pose(np.radians(0.5), (0.1, 0.05, 0.0))
    init = np.ascontiguousarray(np.stack([oracle.pose_compose(bump, base[p][0]) for p in range(n - 1)]))
    d_init = c.alloc(init.nbytes).upload(init)
    res = Q.sequence_dev(c, scans, d_init=d_init.ptr)
    for p in range(n - 1):
        (ea, pa), (eb, pb) = feats[p], feats[p + 1]
        po, to, io = oracle.register_features(scans[p + 1][eb], scans[p + 1][pb], scans[p][ea], scans[p][pa], init[p])
        print(name, p, "oracle", to, io, "gpu", int(res[p]["termination"]), int(res[p]["iterations"]), pose_diff(oracle, po, res[p]["pose"]))
        check_record(oracle, res[p], (po, to, io, None), (name, p, "init"))
    assert not Q.same_bytes(res, Q.sequence_dev(c, scans))  # (the initial poses were really used)
    # the feature-level entry points on one extraction of the same scans
    lidar, fe, reg = Q.lidar(), capi.FeatureExtractionParams(), capi.RegistrationParams()
    ecap, pcap = c.edge_capacity(lidar, fe), c.planar_capacity(lidar, fe)
    d_xyz = c.alloc(scans.nbytes).upload(scans)
    d_ei, d_pi, d_ne, d_np = c.alloc(n * ecap * 4), c.alloc(n * pcap * 4), c.alloc(n * 4), c.alloc(n * 4)
    d_ex, d_px, d_res = c.alloc(n * ecap * 24), c.alloc(n * pcap * 24), c.alloc((n - 1) * 64)
    c.extract_features_batch_dev(d_xyz.ptr, n, lidar, fe, d_ei.ptr, d_ne.ptr, d_ex.ptr, d_pi.ptr, d_np.ptr, d_px.ptr)
    c.register_features_batch_dev(n - 1, d_ex.ptr + ecap * 24, d_ne.ptr + 4, d_px.ptr + pcap * 24, d_np.ptr + 4, d_ex.ptr, d_ne.ptr, d_px.ptr,
                                  d_np.ptr, ecap, pcap, d_init.ptr, reg, d_res.ptr)
    c.synchronize()
    assert Q.same_bytes(d_res.download(capi.RESULT_DTYPE, n - 1), res), name
    for b in (d_xyz, d_ei, d_pi, d_ne, d_np, d_ex, d_px, d_res, d_init):
        b.free()
    with option("STREAM_CHUNK_PAIRS", 3):
        assert Q.same_bytes(c.register_scan_sequence(scans, n, lidar, init=init), res), name


def test_refusals():
    """a NaN in scan 4 makes the host form return LOAMX_ERR_BAD_PARAM and leaves `out` as it was; so does a NaN initial pose;
    the wrapper raises ValueError for arguments that cannot be n_scans scans before anything is copied"""
    c = ctx()
    name, n = Q.SEQUENCES[0]
    scans = Q.sequence(name, n)
    P = n - 1
    sentinel = np.zeros(P, dtype=capi.RESULT_DTYPE)
    sentinel["iterations"] = 77
    bad = scans.copy()
    bad[4, 12345, 1] = np.nan
    for chunk in (0, 3):
        with option("STREAM_CHUNK_PAIRS", chunk), pytest.raises(capi.LoamxError) as e:
            c.register_scan_sequence(bad, n, Q.lidar(), out=sentinel)
        assert e.value.status == capi.ERR_BAD_PARAM
        assert (sentinel["iterations"] == 77).all() and not sentinel["pose"].any()
    init = np.tile(IDENT, (P, 1))
    init[5, 2] = np.nan
    with pytest.raises(capi.LoamxError) as e:
        c.register_scan_sequence(scans, n, Q.lidar(), init=init, out=sentinel)
    assert e.value.status == capi.ERR_BAD_PARAM and (sentinel["iterations"] == 77).all()
    with option("CHECK_FINITE"), pytest.raises(capi.LoamxError) as e:
        Q.sequence_dev(c, bad)
    assert e.value.status == capi.ERR_BAD_PARAM
    good_init = np.tile(IDENT, (P, 1))
    bad_calls = [
        dict(xyz=scans[:, ::2]),                                         # not C-contiguous
        dict(xyz=np.asfortranarray(scans.reshape(-1, 3))),               # Fortran order
        dict(xyz=scans.astype(np.float16)),                              # neither float64 nor float32
        dict(xyz=scans.reshape(-1)[:-1]),                                # one value short
        dict(xyz=scans[:n - 1]),                                         # one scan short
        dict(xyz=(scans.ctypes.data, np.float64)),                       # address without an element count
        dict(xyz=(scans.ctypes.data, np.float64, scans.size - 3)),       # an element count too small
        dict(xyz=(scans.ctypes.data, np.int32, scans.size)),             # address form, wrong dtype
        dict(xyz=scans, out=np.zeros(P, dtype=np.float64)),              # out of the wrong dtype
        dict(xyz=scans, out=sentinel[:P - 1]),                           # out too short
        dict(xyz=scans, init=good_init[:P - 1]),                         # init too short
        dict(xyz=scans, init=good_init.astype(np.float32)),              # init of the wrong dtype
        dict(xyz=scans, init=np.tile(IDENT, (P, 2))[:, :7]),             # init not C-contiguous
        dict(xyz=scans, init=[list(IDENT)] * P),                         # init not an array
    ]
    for kw in bad_calls:
        with pytest.raises(ValueError):
            c.register_scan_sequence(kw["xyz"], n, Q.lidar(), init=kw.get("init"), out=kw.get("out", sentinel))
    assert (sentinel["iterations"] == 77).all()
    # the well-formed forms still run and agree
    good = c.register_scan_sequence(scans, n, Q.lidar())
    assert Q.same_bytes(c.register_scan_sequence((scans.ctypes.data, np.float64, scans.size), n, Q.lidar(), init=good_init), good)
    out = np.zeros(P + 1, dtype=capi.RESULT_DTYPE)
    c.register_scan_sequence(scans, n, Q.lidar(), out=out)
    assert Q.same_bytes(out[:P], good)


def check_trajectory(oracle, c, records, origin):
    """loamx_compose_trajectory_dev against the sequential oracle.pose_compose chain; every pose: rotation within
    1e-14 n rad, translation within 1e-14 n (1 + path length) m — a few roundings of 1.1e-16 per composition with a ~10x
    margin. Two runs: identical bytes."""
    n = len(records)
    d_rec, d_traj = c.alloc(max(n, 1) * 64).upload(records), c.alloc((n + 1) * 56)
    runs = []
    for _ in range(2):
        c.compose_trajectory_dev(d_rec.ptr, n, d_traj.ptr, origin)
        c.synchronize()
        runs.append(d_traj.download(np.float64, (n + 1) * 7).reshape(n + 1, 7).copy())
    d_rec.free(), d_traj.free()
    assert Q.same_bytes(runs[0], runs[1])
    want = [IDENT.copy() if origin is None else np.asarray(origin, dtype=np.float64)]
    for r in records:
        want.append(oracle.pose_compose(want[-1], r["pose"]))
    path = float(np.linalg.norm(records["pose"][:, 4:], axis=1).sum()) if n else 0.0
    worst = (0.0, 0.0)
    for i in range(n + 1):
        rot, trans = pose_diff(oracle, want[i], runs[0][i])
        worst = (max(worst[0], rot), max(worst[1], trans))
        assert rot <= 1e-14 * max(n, 1) and trans <= 1e-14 * max(n, 1) * (1.0 + path), (i, rot, trans)
    assert np.array_equal(runs[0][0], want[0])
    print("trajectory of", n, "poses: worst rotation", worst[0], "translation", worst[1], "path", path)
    return runs[0]


def test_trajectory(oracle):
    c = ctx()
    name, n = Q.SEQUENCES[0]
    res = Q.sequence_dev(c, Q.sequence(name, n))
    origin = oracle.pose_compose(S.yaw_pose(0.7, (12.0, -3.0, 1.8)), np.array([np.sin(0.1), 0, 0, np.cos(0.1), 0.3, 0, 0]))  # (not about z alone)
    for o in (None, origin):
        traj = check_trajectory(oracle, c, res, o)
        assert np.linalg.norm(traj[-1][4:] - traj[0][4:]) > 0.5 * 0.8 * (n - 1)  # (the drive: 0.8 m per scan)
    # a long synthetic drive: small random motions, uploaded as records
    rng = np.random.default_rng(2024)
    m = 4096
    rec = np.zeros(m, dtype=capi.RESULT_DTYPE)
    axis = rng.normal(size=(m, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = rng.uniform(-0.02, 0.02, m)
    rec["pose"][:, :3] = axis * np.sin(ang / 2)[:, None]
    rec["pose"][:, 3] = np.cos(ang / 2)
    rec["pose"][:, 4:] = rng.uniform(-0.5, 0.5, (m, 3)) + np.array([0.8, 0.0, 0.0])
    rec["termination"] = rng.integers(0, 3, m)  # (a pair that ended INSUFFICIENT_ASSOCIATIONS is composed like any other)
    for o in (None, origin):
        check_trajectory(oracle, c, rec, o)
    check_trajectory(oracle, c, rec[:0], origin)  # no pairs: the origin alone
    check_trajectory(oracle, c, rec[:65], None)   # one record into the second tile of 64
    # both sides of every edge of the first two tiles of 64 records, and the shortest chains
    for k in (1, 2, 63, 64, 127, 128, 129):
        for o in (None, origin):
            check_trajectory(oracle, c, rec[:k], o)
