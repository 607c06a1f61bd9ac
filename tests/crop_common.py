"""The rule of the map window (include/loamx.h, "map window") in plain numpy, float64 operations one at a time in the header's
order, so everything is compared by equality; the crop of the three map models (cloudmap_common, surfel_common,
occupancy_common: entries deleted from their dicts, whose insertion order IS the list order); the table's home slot and a search
for keys that share one. No code shared with the kernels. Also: the binding of tests/hostcheck_crop (crop_math.h compiled by g++
as a program of its own)."""
import os
import subprocess
import tempfile

import numpy as np

import cloudmap_common as CM

BIAS = CM.BIAS
HASH_MUL = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


def crop_bounds(pose, lo, hi, leaf):
    """(skip, flo (3,), fhi (3,)): pose is 7 numbers or None (the centre is +0.0)"""
    c = np.zeros(3) if pose is None else np.asarray(pose, dtype=np.float64)[4:7]
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    skip = not bool(np.isfinite(c).all())
    with np.errstate(all="ignore"):
        flo = np.floor((c + lo) / leaf)
        fhi = np.floor((c + hi) / leaf)
    return skip, flo, fhi


def key_cell(key):
    key = int(key)
    return [((key >> s) & 0x1FFFFF) - BIAS for s in (42, 21, 0)]


def keeps(key, flo, fhi):
    v = key_cell(key)
    return all(float(v[a]) >= flo[a] and float(v[a]) <= fhi[a] for a in range(3))


def model_leaf(model):
    return model.p["leaf"] if hasattr(model, "p") else model.leaf


def crop_model(model, pose, lo, hi):
    """deletes the voxels the rule removes from a CloudMapModel, SurfelMapModel or OccupancyModel -> (kept, removed, skipped)"""
    vox = model.vox
    skip, flo, fhi = crop_bounds(pose, lo, hi, model_leaf(model))
    if skip:
        return len(vox), 0, 1
    gone = [k for k in vox if not keeps(k, flo, fhi)]
    for k in gone:
        del vox[k]
    if hasattr(model, "st"):
        model.st["voxels"] = len(vox)
    return len(vox), len(gone), 0


def home_slot(key, log2_cap):
    return ((int(key) * HASH_MUL) & M64) >> (64 - log2_cap)


def table_log2(slots_min):
    """voxel_table_log2 of the library: at least 4 bits"""
    l = 4
    while (1 << l) < slots_min:
        l += 1
    return l


def colliding_cells(n, log2_cap, reach=4096):
    """n cells (x, 0, 0), x = 1, 2, ... ascending, whose keys share one home slot: the first slot that n cells of the row fall into"""
    by_slot = {}
    for x in range(1, reach + 1):
        cells_of = by_slot.setdefault(home_slot(cell_key((x, 0, 0)), log2_cap), [])
        cells_of.append((x, 0, 0))
        if len(cells_of) == n:
            return cells_of
    raise AssertionError("no collision found")


def cell_key(cell):
    return int(CM.pack(np.array([cell], dtype=np.int64))[0])


# ---- the clouds of the comparison with the models (tests/test_gpu_crop.py) and of the layers above the C ABI (tests/test_gpu_crop_modules.py)
def posed_clouds(seed, sizes, centre=(0.0, 0.0, 0.0)):
    """(points, offsets, poses): clouds of points a few metres around sensors near `centre`"""
    rng = np.random.default_rng(seed)
    n = sum(sizes)
    pts = rng.uniform(-3.0, 3.0, (n, 3)) * [1.0, 1.0, 0.25]
    poses = []
    for _ in sizes:
        q = np.array([0.0, 0.0, np.sin(rng.uniform(-0.5, 0.5)), 1.0])
        q[3] = np.cos(np.arcsin(q[2]))
        poses.append(np.concatenate([q, np.asarray(centre) + rng.uniform(-1.5, 1.5, 3) * [1.0, 1.0, 0.1]]))
    return pts, np.concatenate([[0], np.cumsum(sizes)]), np.stack(poses)


CASE3_CENTRE = (0.3, -0.2, 0.1)
CASE3_BOXES = (([-10.0, -10.0, -10.0], [0.0, 10.0, 10.0]), ([-np.inf, -1.05, -np.inf], [np.inf, 2.0, 0.3]))


def case3_clouds():
    """((points, offsets, poses) of three posed clouds of about 5 000 points, the same of a fourth cloud over what the first box removes)"""
    return posed_clouds(61, (1700, 1800, 1500)), posed_clouds(62, (1400,), centre=(2.5, 0.0, 0.0))


# ---- tests/hostcheck_crop: crop_math.h compiled by g++ ----------------------------------------------------------------------------
HOSTCHECK_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck_crop")
CROP_IN = np.dtype([("c", np.float64, 3), ("lo", np.float64, 3), ("hi", np.float64, 3), ("leaf", np.float64), ("key", np.uint64)])
CROP_OUT = np.dtype([("skip", np.uint64), ("flo", np.float64, 3), ("fhi", np.float64, 3), ("keep", np.uint64)])
assert CROP_IN.itemsize == 88 and CROP_OUT.itemsize == 64


def hostcheck_program(san=False):
    subprocess.check_call(["make", "-s", "-C", HOSTCHECK_DIR] + (["san"] if san else []))
    return os.path.join(HOSTCHECK_DIR, "hostcheck_crop_san" if san else "hostcheck_crop")


def hostcheck_run(program, records):
    """CROP_OUT per CROP_IN record"""
    records = np.ascontiguousarray(records, dtype=CROP_IN)
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        records.tofile(fin)
        r = subprocess.run([program, fin, fout], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        out = np.fromfile(fout, dtype=CROP_OUT)
    assert len(out) == len(records)
    return out
