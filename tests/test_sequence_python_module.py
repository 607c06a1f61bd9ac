"""GPU: the two extensions of the pybind11 module `loam` — registerScanSequence and deskewScan — against the ctypes
binding of the same C ABI entry points."""
import os
import sys

import numpy as np
import pytest

import sequence_common as Q
from gpu_common import ctx
from loam_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _loam():
    B.build_pybind()
    p = os.path.join(ROOT, "loam_amd", "python")
    if p not in sys.path:
        sys.path.insert(0, p)
    import loam
    return loam


def pose7(p):
    r = p.rotation
    return np.array([r.x(), r.y(), r.z(), r.w(), *p.translation])


def test_register_scan_sequence_equals_the_capi_records():
    loam = _loam()
    name, n = Q.SEQUENCES[0]
    scans = Q.sequence(name, n)
    lp = loam.LidarParams(scan_lines=Q.H, points_per_line=Q.W, min_range=1.0, max_range=120.0)
    want = ctx().register_scan_sequence(scans, n, Q.lidar())
    got = loam.registerScanSequence(scans, lp)
    assert len(got) == n - 1
    assert np.array_equal(np.stack([pose7(p) for p in got]), want["pose"])
    # float32 scans take the f32 entry point; keyword arguments; initial poses
    s32 = np.ascontiguousarray(scans.astype(np.float32))
    want32 = ctx().register_scan_sequence(s32, n, Q.lidar())
    got32 = loam.registerScanSequence(scans=s32, lidar_params=lp, fe_params=loam.FeatureExtractionParams(),
                                      reg_params=loam.RegistrationParams())
    assert np.array_equal(np.stack([pose7(p) for p in got32]), want32["pose"])
    assert not np.array_equal(want32["pose"], want["pose"])
    init = np.ascontiguousarray(want["pose"].copy())
    init[:, 4] += 0.05
    inits = [loam.Pose3d(loam.Quaterniond(q[3], q[0], q[1], q[2]), q[4:]) for q in init]
    want_i = ctx().register_scan_sequence(scans, n, Q.lidar(), init=init)
    got_i = loam.registerScanSequence(scans, lp, inits=inits)
    assert np.array_equal(np.stack([pose7(p) for p in got_i]), want_i["pose"])
    assert loam.registerScanSequence(scans[:1], lp) == []
    with pytest.raises(RuntimeError):
        loam.registerScanSequence(scans[:, :-1], lp)       # scans of the wrong size
    with pytest.raises(RuntimeError):
        loam.registerScanSequence(scans, lp, inits=inits[:-1])


def test_deskew_scan_equals_the_capi():
    loam = _loam()
    name, n = Q.SEQUENCES[0]
    scans = Q.sequence(name, n)
    lp = loam.LidarParams(scan_lines=Q.H, points_per_line=Q.W, min_range=1.0, max_range=120.0)
    m = ctx().register_scan_sequence(scans[:2], 2, Q.lidar())["pose"][0]
    motion = loam.Pose3d(loam.Quaterniond(m[3], m[0], m[1], m[2]), m[4:])
    for rho in (1.0, 0.5):
        for data in (scans[1], np.ascontiguousarray(scans[1].astype(np.float32))):
            want = ctx().deskew_scans(data, Q.lidar(), m, rho)
            got = loam.deskewScan(data, lp, motion, ref_fraction=rho)
            assert got.dtype == data.dtype and got.shape == (Q.N, 3)
            assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (rho, data.dtype)
    assert np.array_equal(loam.deskewScan(scans[1], lp, loam.Pose3d.Identity()), scans[1])
    with pytest.raises(RuntimeError):
        loam.deskewScan(scans[1], lp, motion, ref_fraction=1.5)
