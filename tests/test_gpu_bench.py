"""GPU: a plain `bench.py` run prints the headline line only, and `--dump-outputs` writes the records the timed path
returned in its last step: the same bits as one loamx_register_scan_pairs_dev call on the same seeded pairs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_common import ctx
from loam_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, SEED, P = 64, 1024, 20240311, 8  # the bench scans (bench.py), a small batch


def test_plain_run_dumps_what_the_path_computes(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--pairs", str(P), "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert k in line
    for k in ("roofline", "kernels", "results", "cpu_baseline", "parity", "extra"):
        assert k not in line  # (--full only)

    c = ctx()
    d_xyz, d_res = c.alloc(P * 2 * H * W * 24), c.alloc(P * 64)
    c.synth_scan_pairs_dev(SEED, 0, P, H, W, 0.01, d_xyz.ptr)
    c.register_scan_pairs_dev(d_xyz.ptr, P, capi.LidarParams(H, W, 1.0, 120.0), capi.FeatureExtractionParams(),
                              capi.RegistrationParams(), d_res.ptr)
    c.synchronize()
    want = d_res.download(np.uint8, P * 64).copy().view(capi.RESULT_DTYPE)
    d_xyz.free()
    d_res.free()

    got = {n: np.load(os.path.join(tmp_path, n + ".npy")) for n in ("pose", "termination", "iterations")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["pose"].shape == (P, 7) and got["termination"].shape == (P,) and got["iterations"].shape == (P,)
    assert np.array_equal(got["pose"].view(np.uint64), want["pose"].view(np.uint64))
    assert np.array_equal(got["termination"], want["termination"].astype(np.float64))
    assert np.array_equal(got["iterations"], want["iterations"].astype(np.float64))
    assert (want["termination"] == capi.CONVERGED).all()
