"""GPU: the entry points of the registration information matrix against each other, byte for byte.
  * loamx_registration_information_batch_dev on five pairs of different sizes equals the host single-pair form pair by pair,
    twice, and under DEBUG_POISON and QUEUE_TWO_STAGE;
  * the indexed form on a grid-searched target equals the plain form;
  * the "_info_dev" pair and sequence forms (FP64 and f32): result records of the plain forms, information records of the
    batch form at the records' poses on the features of loamx_extract_features_batch_dev — also where every pair stops in
    iteration 0 (the early return) and with one iteration;
  * refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

import info_common as I
from gpu_common import ctx, option
from loam_amd import capi
from test_gpu_information import IDENT, room

pytestmark = pytest.mark.gpu

H, W, N, SEED = 16, 256, 16 * 256, 3
REC = capi.INFORMATION_DTYPE


def lidar():
    return capi.LidarParams(H, W, 1.0, 120.0)


def upload_sets(c, sets, stride):
    """feature sets of P pairs -> one device array [P][stride][3] and the counts"""
    buf = np.zeros((len(sets), stride, 3))
    for p, s in enumerate(sets):
        buf[p, :len(s)] = s
    return c.alloc(max(buf.nbytes, 8)).upload(buf), c.alloc(4 * len(sets)).upload(np.array([len(s) for s in sets], dtype=np.uint32))


def batch_information(c, pairs, poses, reg=None):
    """pairs: [(src_edge, src_planar, tgt_edge, tgt_planar)] -> INFORMATION_DTYPE records of ONE batch call"""
    reg = reg or capi.RegistrationParams()
    P = len(pairs)
    es = max(max(len(p[0]), len(p[2])) for p in pairs)
    ps = max(max(len(p[1]), len(p[3])) for p in pairs)
    bufs = []
    try:
        d = [upload_sets(c, [p[k] for p in pairs], es if k % 2 == 0 else ps) for k in range(4)]
        bufs = [b for pair in d for b in pair]
        d_pose, d_info = c.alloc(P * 56).upload(np.ascontiguousarray(poses, dtype=np.float64)), c.alloc(P * REC.itemsize)
        bufs += [d_pose, d_info]
        c.registration_information_batch_dev(P, d[0][0].ptr, d[0][1].ptr, d[1][0].ptr, d[1][1].ptr, d[2][0].ptr, d[2][1].ptr, d[3][0].ptr,
                                             d[3][1].ptr, es, ps, d_pose.ptr, reg, d_info.ptr)
        c.synchronize()
        return d_info.download(REC, P).copy()
    finally:
        for b in bufs:
            b.free()


def host_record(c, pair, pose, reg=None):
    info = c.registration_information(*pair, pose=pose, reg=reg)
    return np.frombuffer(bytes(info), dtype=REC)[0]


def corridor_with(n_tgt_slices):
    """the corridor of info_common with another number of target slices (121: 484 target edge points)"""
    se, sp, _, _ = I.corridor()
    tgt = [I._slice(y, 0.0) for y in np.linspace(-15.0, 15.0, n_tgt_slices)]
    return se, sp, np.concatenate([s[0] for s in tgt]), np.concatenate([s[1] for s in tgt])


@functools.lru_cache(maxsize=None)
def five_pairs(oracle):
    se, sp, te, tp, _ = room(oracle, H, W)
    far = np.array([0, 0, 0, 1.0, 500.0, -300.0, 40.0])
    pairs = [(se, sp, te, tp), (np.zeros((0, 3)), sp, te, tp), corridor_with(161), corridor_with(121), (se, sp, te, tp)]
    poses = np.stack([IDENT, IDENT, IDENT, IDENT, far])
    assert len(pairs[2][2]) == 644 > 512 >= len(pairs[3][2]) == 484  # a target edge set on each side of kBruteMax
    return pairs, poses


@pytest.mark.parametrize("opt", [None, "DEBUG_POISON", "QUEUE_TWO_STAGE"])
def test_batch_of_five_equals_the_host_form_pair_by_pair(oracle, opt):
    c = ctx()
    pairs, poses = five_pairs(oracle)
    plain = batch_information(c, pairs, poses)
    assert plain["n_edge"].tolist()[1] == 0 and plain["n_edge"][0] > 30 and plain["n_plane"][1] == plain["n_plane"][0] > 500
    assert plain["n_edge"][2] == plain["n_edge"][3] == 196 and plain["n_plane"][2] == 1568
    # too far apart to associate at all: a zero matrix, zero eigenvalues, identity eigenvectors
    z = plain[4]
    assert (int(z["n_edge"]), int(z["n_plane"]), int(z["n_dropped"])) == (0, 0, 0) and not z["information"].any() and not z["eigenvalues"].any()
    assert np.array_equal(z["eigenvectors"], np.eye(6)) and not z["gradient"].any() and z["weighted_sq_error"] == 0
    with option(opt) if opt else option("DEBUG_POISON", 0):
        batch = batch_information(c, pairs, poses)
        again = batch_information(c, pairs, poses)
        singles = np.array([host_record(c, pair, pose) for pair, pose in zip(pairs, poses)], dtype=REC)
    assert batch.tobytes() == again.tobytes()
    for p in range(len(pairs)):
        assert batch[p].tobytes() == singles[p].tobytes(), (opt, p)
    assert batch.tobytes() == plain.tobytes()  # (the switches change no result)
    # and in another batch: the pairs in reverse order
    rev = batch_information(c, pairs[::-1], poses[::-1])
    assert rev[::-1].tobytes() == plain.tobytes()


def test_indexed_form_equals_the_plain_form(oracle):
    c = ctx()
    se, sp, te, tp, registered = room(oracle, H, W)
    assert len(tp) > 512  # searched through its grid
    index = c.target_index(te, tp)
    try:
        for pose in (IDENT, registered):
            a = c.registration_information_indexed(index, se, sp, pose=pose)
            b = c.registration_information(se, sp, te, tp, pose=pose)
            assert bytes(a) == bytes(b) and int(a.n_plane) > 500
    finally:
        c.target_index_destroy(index)


def extracted_features(c, d_xyz, n_scans, f32):
    """loamx_extract_features_batch_dev over the scans: device buffers (edge xyz, n edge, planar xyz, n planar), capacities"""
    fe = capi.FeatureExtractionParams()
    ecap, pcap = c.edge_capacity(lidar(), fe), c.planar_capacity(lidar(), fe)
    d_e, d_ne, d_p, d_np = c.alloc(n_scans * ecap * 24), c.alloc(n_scans * 4), c.alloc(n_scans * pcap * 24), c.alloc(n_scans * 4)
    c.extract_features_batch_dev(d_xyz, n_scans, lidar(), fe, None, d_ne.ptr, d_e.ptr, None, d_np.ptr, d_p.ptr, f32=f32)
    c.synchronize()
    return (d_e, d_ne, d_p, d_np), ecap, pcap


def scans_of(f32):
    A, B = capi.synth_scan_host(SEED, 2, 0, H, W, 0.01), capi.synth_scan_host(SEED, 2, 1, H, W, 0.01)
    A1, B1 = capi.synth_scan_host(SEED, 5, 0, H, W, 0.01), capi.synth_scan_host(SEED, 5, 1, H, W, 0.01)
    pairs = np.ascontiguousarray(np.stack([A, B, A1, B1, B, A]).reshape(3, 2, N, 3))  # three pairs, target first
    seq = np.ascontiguousarray(np.stack([A, B, A, B]))                                   # four scans: pairs (A, B), (B, A), (A, B)
    return (pairs.astype(np.float32), seq.astype(np.float32)) if f32 else (pairs, seq)


REGS = {"default": {}, "early return": {"min_associations": 10 ** 9}, "one iteration": {"max_iterations": 1}}


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("case", list(REGS))
def test_scan_pair_and_sequence_info_forms(f32, case):
    c = ctx()
    reg = capi.RegistrationParams()
    for k, v in REGS[case].items():
        setattr(reg, k, v)
    fe = capi.FeatureExtractionParams()
    pairs, seq = scans_of(f32)
    bufs = []
    try:
        # ---- interleaved pairs
        P = len(pairs)
        d_xyz, d_res, d_res2, d_info = c.alloc(pairs.nbytes).upload(pairs), c.alloc(P * 64), c.alloc(P * 64), c.alloc(P * REC.itemsize)
        bufs += [d_xyz, d_res, d_res2, d_info]
        c.register_scan_pairs_dev(d_xyz.ptr, P, lidar(), fe, reg, d_res.ptr, f32=f32)
        c.register_scan_pairs_dev(d_xyz.ptr, P, lidar(), fe, reg, d_res2.ptr, f32=f32, d_info=d_info.ptr)
        c.synchronize()
        res, res2, info = d_res.download(capi.RESULT_DTYPE, P), d_res2.download(capi.RESULT_DTYPE, P), d_info.download(REC, P)
        assert res.tobytes() == res2.tobytes()
        if case == "early return":
            assert (res["termination"] == capi.INSUFFICIENT_ASSOCIATIONS).all() and (res["iterations"] == 0).all()
            assert all(np.array_equal(r["pose"], IDENT) for r in res)
        elif case == "one iteration":
            assert (res["iterations"] == 1).all()
        else:
            assert (res["iterations"] >= 2).all()
        assert (info["n_plane"] > 500).all() and (info["n_edge"] > 20).all()  # records were written, at poses that associate
        feats, ecap, pcap = extracted_features(c, d_xyz.ptr, 2 * P, f32)
        bufs += list(feats)
        e = feats[0].download(np.float64, 2 * P * ecap * 3).reshape(2 * P, ecap, 3)
        pl = feats[2].download(np.float64, 2 * P * pcap * 3).reshape(2 * P, pcap, 3)
        ne, npl = feats[1].download(np.uint32, 2 * P), feats[3].download(np.uint32, 2 * P)
        sets = [(e[2 * p + 1, :ne[2 * p + 1]], pl[2 * p + 1, :npl[2 * p + 1]], e[2 * p, :ne[2 * p]], pl[2 * p, :npl[2 * p]]) for p in range(P)]
        want = batch_information(c, sets, res["pose"], reg)
        assert info.tobytes() == want.tobytes()
        # ---- sequence: pair p = (scan p target, scan p + 1 source); the batch form reads the source sets by pointer offset
        S = len(seq)
        d_seq, d_sres, d_sres2, d_sinfo = c.alloc(seq.nbytes).upload(seq), c.alloc((S - 1) * 64), c.alloc((S - 1) * 64), c.alloc((S - 1) * REC.itemsize)
        bufs += [d_seq, d_sres, d_sres2, d_sinfo]
        c.register_scan_sequence_dev(d_seq.ptr, S, lidar(), fe, reg, d_sres.ptr, f32=f32)
        c.register_scan_sequence_dev(d_seq.ptr, S, lidar(), fe, reg, d_sres2.ptr, f32=f32, d_info=d_sinfo.ptr)
        c.synchronize()
        sres, sres2, sinfo = d_sres.download(capi.RESULT_DTYPE, S - 1), d_sres2.download(capi.RESULT_DTYPE, S - 1), d_sinfo.download(REC, S - 1)
        assert sres.tobytes() == sres2.tobytes()
        assert (sinfo["n_plane"] > 500).all()
        sf, ecap, pcap = extracted_features(c, d_seq.ptr, S, f32)
        bufs += list(sf)
        d_pose, d_want = c.alloc((S - 1) * 56).upload(np.ascontiguousarray(sres["pose"])), c.alloc((S - 1) * REC.itemsize)
        bufs += [d_pose, d_want]
        c.registration_information_batch_dev(S - 1, sf[0].ptr + ecap * 24, sf[1].ptr + 4, sf[2].ptr + pcap * 24, sf[3].ptr + 4, sf[0].ptr, sf[1].ptr,
                                             sf[2].ptr, sf[3].ptr, ecap, pcap, d_pose.ptr, reg, d_want.ptr)
        c.synchronize()
        assert sinfo.tobytes() == d_want.download(REC, S - 1).tobytes()
        assert sinfo[0].tobytes() == info[0].tobytes() == sinfo[2].tobytes()  # the same pair in three places
    finally:
        for b in bufs:
            b.free()


def test_refusals(oracle):
    c = ctx()
    se, sp, te, tp, _ = room(oracle, H, W)
    reg = capi.RegistrationParams()
    info = capi.RegInformation()
    dp = C.POINTER(C.c_double)
    arg = lambda a: a.ctypes.data_as(dp)
    pose = IDENT.copy()
    call = lambda **kw: c.lib.loamx_registration_information(
        c.h, kw.get("se", arg(se)), len(se), arg(sp), len(sp), arg(te), len(te), kw.get("tp", arg(tp)), len(tp), kw.get("pose", arg(pose)),
        kw.get("reg", C.byref(reg)), kw.get("info", C.byref(info)))
    assert call() == capi.OK
    for null in ("se", "tp", "pose", "reg", "info"):
        assert call(**{null: None}) == capi.ERR_BAD_PARAM, null
    assert c.lib.loamx_registration_information(None, arg(se), len(se), arg(sp), len(sp), arg(te), len(te), arg(tp), len(tp), arg(pose),
                                                C.byref(reg), C.byref(info)) == capi.ERR_BAD_PARAM
    nan_pose = IDENT.copy()
    nan_pose[5] = np.nan
    assert call(pose=arg(nan_pose)) == capi.ERR_BAD_PARAM
    bad = se.copy()
    bad[3, 1] = np.inf
    assert call(se=arg(bad)) == capi.ERR_BAD_PARAM
    for field in ("num_edge_neighbors", "num_plane_neighbors"):
        r = capi.RegistrationParams()
        setattr(r, field, 17)
        with pytest.raises(capi.LoamxError) as e:
            c.registration_information(se, sp, te, tp, reg=r)
        assert e.value.status == capi.ERR_UNSUPPORTED
    # the indexed and device forms
    assert c.lib.loamx_registration_information_indexed(c.h, None, arg(se), len(se), arg(sp), len(sp), arg(pose), C.byref(reg), C.byref(info)) == capi.ERR_BAD_PARAM
    assert c.lib.loamx_registration_information_batch_dev(c.h, 1, None, None, None, None, None, None, None, None, 8, 8, None, C.byref(reg), None) == capi.ERR_BAD_PARAM
    d = c.alloc(64)
    try:
        assert c.lib.loamx_register_scan_pairs_info_dev(c.h, d.ptr, 1, C.byref(lidar()), C.byref(capi.FeatureExtractionParams()), C.byref(reg), d.ptr, None) == capi.ERR_BAD_PARAM
        assert c.lib.loamx_register_scan_sequence_info_dev(c.h, d.ptr, 2, C.byref(lidar()), C.byref(capi.FeatureExtractionParams()), C.byref(reg), None, d.ptr, None) == capi.ERR_BAD_PARAM
    finally:
        d.free()
    # max_iterations plays no part: 0 is accepted and gives the record of the default
    r0 = capi.RegistrationParams()
    r0.max_iterations = 0
    assert bytes(c.registration_information(se, sp, te, tp, reg=r0)) == bytes(c.registration_information(se, sp, te, tp))
    assert int(c.registration_information(se, sp, te, tp, reg=r0).n_plane) > 500
