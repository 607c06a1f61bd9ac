"""Shared inputs of the scan-sequence and de-skew tests: short drives through the outdoor scenes (tests/outdoor_scenes.py)
and what the oracle makes of their consecutive pairs."""
import functools

import numpy as np

import outdoor_scenes as S
from loam_amd import capi

H, W = 64, 1024
N = H * W
SEQUENCES = (("canyon", 9), ("lot", 5))


def lidar():
    return capi.LidarParams(H, W, 1.0, 120.0)


@functools.lru_cache(maxsize=None)
def sequence(name, n):
    """n consecutive 64 x 1024 scans of a drive: 0.8 m forward per scan with a small sideways weave, 0.006 rad of heading
    per scan; (n, N, 3) float64"""
    o0, yaw0 = S.sensor_origin(name, 3)
    scans = []
    for i in range(n):
        origin = o0 + 0.8 * i * np.array([np.cos(yaw0), np.sin(yaw0), 0.0]) + np.array([0.0, 0.05 * np.sin(i), 0.0])
        scans.append(S.scan_at(name, 0, origin, yaw0 + 0.006 * i, H, W, 0.01, noise_seed=1000 + i))
    out = np.ascontiguousarray(np.stack(scans))
    out.setflags(write=False)
    return out


def widened(scans):
    return scans.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def oracle_features(oracle, name, n, f32=False):
    """per scan (edge idx, planar idx) of the oracle's extraction (f32: of the scans rounded to float and widened)"""
    scans = widened(sequence(name, n)) if f32 else sequence(name, n)
    return [oracle.extract_features(s, H, W, 1.0, 120.0) for s in scans]


@functools.lru_cache(maxsize=None)
def oracle_pairs(oracle, name, n, f32=False):
    """per consecutive pair (pose, termination, iterations, info) of the oracle: target scan p, source scan p + 1, identity
    initial pose"""
    scans = widened(sequence(name, n)) if f32 else sequence(name, n)
    feats = oracle_features(oracle, name, n, f32)
    out = []
    for p in range(n - 1):
        (ea, pa), (eb, pb) = feats[p], feats[p + 1]
        out.append(oracle.register_features(scans[p + 1][eb], scans[p + 1][pb], scans[p][ea], scans[p][pa], want_info=True))
    return out


def duplicated(scans):
    """the pair entry points' layout of the same pairs: [(scan p, scan p + 1)], target first"""
    return np.ascontiguousarray(np.stack([scans[:-1], scans[1:]], axis=1))


def sequence_dev(c, scans, reg=None, d_init=0, fe=None):
    """loamx_register_scan_sequence_dev[_f32] on host scans: upload, run, download the n - 1 records"""
    n = len(scans)
    fe, reg = fe or capi.FeatureExtractionParams(), reg or capi.RegistrationParams()
    d_xyz, d_res = c.alloc(scans.nbytes).upload(scans), c.alloc(max(n - 1, 1) * 64)
    try:
        c.register_scan_sequence_dev(d_xyz.ptr, n, lidar(), fe, reg, d_res.ptr, d_init=d_init, f32=scans.dtype == np.float32)
        c.synchronize()
        return d_res.download(capi.RESULT_DTYPE, n - 1).copy()
    finally:
        d_xyz.free(), d_res.free()


def pairs_dev(c, pairs, reg=None, fe=None):
    """loamx_register_scan_pairs_dev[_f32] on a host (P, 2, N, 3) array"""
    P = len(pairs)
    fe, reg = fe or capi.FeatureExtractionParams(), reg or capi.RegistrationParams()
    d_xyz, d_res = c.alloc(pairs.nbytes).upload(pairs), c.alloc(P * 64)
    try:
        c.register_scan_pairs_dev(d_xyz.ptr, P, lidar(), fe, reg, d_res.ptr, f32=pairs.dtype == np.float32)
        c.synchronize()
        return d_res.download(capi.RESULT_DTYPE, P).copy()
    finally:
        d_xyz.free(), d_res.free()


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
