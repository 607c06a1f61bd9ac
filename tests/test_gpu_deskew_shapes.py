"""GPU: deskew_kernel<T> (loam_amd/csrc/sequence_kernels.hip) at every form of its line loop. One thread owns a column of a scan
and walks its workgroup's share of the scan lines, `unroll` (4) lines in flight; launch_deskew splits the lines into shares. The
other de-skew tests run 64 x 1024 scans, where a share is one line: the loop body runs once with u = 0. Here the shapes reach the
four-lines-in-flight body, its remainder, a last share shorter than the others and a last column block narrower than 256, and
every case ASSERTS its form from loamx_deskew_launch_geometry — the launcher's own function — so that a later change of the
launcher fails the test instead of quietly moving a case onto another form.

Reference and allowance are those of test_gpu_deskew.py: deskew_numpy and bound() = 1e-12 (1 + |p| + |t|) m. Points are uniform
in (-100, 100)^3 and every scan has its own motion (angle 1e-3, 0.3, 2.0 or pi - 1e-9 about a random axis, t in (-5, 5)^3, every
fourth quaternion scaled by -3), so a point attributed to the wrong scan, line or column is off by millimetres to metres.
(deskew_numpy itself, against 40-digit arithmetic on such inputs, stays below 1e-3 of bound().)"""
import functools

import numpy as np
import pytest

from gpu_common import ctx
from loam_amd import capi
from test_gpu_deskew import bound, deskew_numpy

pytestmark = pytest.mark.gpu

BLOCK = 256  # columns per column block (asserted below through the last block's width)
# scans, H, W | column blocks, lines per share, shares, lines in the last share, columns in the last block
CASES = [
    (5, 1, 1, 1, 1, 1, 1, 1),
    (1, 1, 257, 2, 1, 1, 1, 1),
    (1, 4096, 100, 1, 2, 2048, 2, 100),
    (1, 4099, 37, 1, 3, 1367, 1, 37),
    (40, 16, 1800, 8, 3, 6, 1, 8),
    (64, 71, 300, 2, 5, 15, 1, 44),
    (2048, 8, 16, 1, 8, 1, 8, 16),
    (2048, 9, 16, 1, 9, 1, 9, 16),
    (300, 64, 64, 1, 10, 7, 4, 64),
    (9, 128, 2048, 8, 5, 26, 3, 256),
]
RHOS = (0.0, 0.37, 1.0)
ANGLES = (1e-3, 0.3, 2.0, np.pi - 1e-9)
KINDS = np.array([[0.0, 0.0, 0.0], [np.nan, 1.0, 2.0], [3.0, -np.inf, 2.0]])
GUARD = 4096
PATTERN = 0xA5
_worst = {}


def case_id(k):
    return "%dx%dx%d" % CASES[k][:3]


def measured(k):
    """the case's form as the launcher's own function gives it, in the order of the CASES columns"""
    n, h, w = CASES[k][:3]
    g = capi.deskew_launch_geometry(n, h, w)
    return g, (g.col_blocks, g.lines_per_share, g.shares, h - (g.shares - 1) * g.lines_per_share, w - (g.col_blocks - 1) * BLOCK)


def uniq(seq):
    return list(dict.fromkeys(int(v) for v in seq))


def placement(k):
    """the pass-through points of a case, {(scan, line, column): kind}, and how many of them lie in each slot of the loop. In three
    scans: on lines that a thread holds in slot u = 1, 2, 3 (the first and the last such line of the scan) and on the last line of
    the last share; a column of its own per slot, so that the neighbours in line and column stay live"""
    n, h, w = CASES[k][:3]
    g = capi.deskew_launch_geometry(n, h, w)
    lines = np.arange(h)
    slot = (lines % g.lines_per_share) % g.unroll
    cols = uniq([0, w - 1, w // 2, w // 3])  # (four columns, no two adjacent, once W >= 9)
    assert (g.shares - 1) * g.lines_per_share <= h - 1 < g.shares * g.lines_per_share  # (line h - 1 IS in the last share)
    special = {}
    for i, s in enumerate(uniq([0, n // 2, n - 1])):
        for j, u in enumerate((1, 2, 3)):
            at = lines[slot == u]
            for l in (uniq(at[[0, -1]]) if len(at) else []):
                special[(s, l, cols[j % len(cols)])] = (i + j) % 3
        special[(s, h - 1, cols[3 % len(cols)])] = (i + 3) % 3
    return special, {u: sum(1 for (_, l, _) in special if slot[l] == u) for u in range(4)}


@functools.lru_cache(maxsize=2)
def inputs(k):
    """scans (n, H * W, 3), motions (n, 7), both read-only; the pass-through points [(scan, line, column)]; their count per slot"""
    n, h, w = CASES[k][:3]
    rng = np.random.default_rng(1000 + k)
    xyz = rng.uniform(-100.0, 100.0, (n, h * w, 3))
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    angle = np.array([ANGLES[(s + k) % 4] for s in range(n)])
    motions = np.concatenate([axis * np.sin(angle / 2)[:, None], np.cos(angle / 2)[:, None], rng.uniform(-5.0, 5.0, (n, 3))], axis=1)
    motions[(np.arange(n) + k) % 4 == 3, :4] *= -3.0
    special, slots = placement(k)
    grid = xyz.reshape(n, h, w, 3)
    for (s, l, c), kind in special.items():
        grid[s, l, c] = KINDS[kind]
    xyz.setflags(write=False), motions.setflags(write=False)
    return xyz, motions, tuple(special), slots


class Dev:
    """the case's scans and motions on the device, an output buffer with GUARD bytes of PATTERN at each end"""

    def __init__(self, c, data, motions):
        self.c, self.data = c, np.ascontiguousarray(data)
        self.bits = np.uint64 if data.dtype == np.float64 else np.uint32
        self.d_in = c.alloc(data.nbytes).upload(self.data)
        self.d_m = c.alloc(motions.nbytes).upload(motions)
        self.d_out = c.alloc(data.nbytes + 2 * GUARD)

    def out_of_place(self, lidar, rho):
        c, data = self.c, self.data
        self.d_out.upload(np.full(data.nbytes + 2 * GUARD, PATTERN, dtype=np.uint8))
        c.deskew_scans_dev(self.d_in.ptr, len(data), lidar, self.d_m.ptr, self.d_out.ptr + GUARD, rho, f32=data.dtype == np.float32)
        c.synchronize()
        raw = self.d_out.download(np.uint8, data.nbytes + 2 * GUARD)
        assert (raw[:GUARD] == PATTERN).all() and (raw[-GUARD:] == PATTERN).all(), "the kernel wrote outside its output"
        assert np.array_equal(self.d_in.download(self.bits, data.size), data.view(self.bits).reshape(-1)), "the kernel wrote its input"
        return raw[GUARD:-GUARD].view(data.dtype).reshape(data.shape)

    def in_place(self, lidar, rho):
        c, data = self.c, self.data
        d = c.alloc(data.nbytes).upload(data)
        c.deskew_scans_dev(d.ptr, len(data), lidar, self.d_m.ptr, d.ptr, rho, f32=data.dtype == np.float32)
        c.synchronize()
        out = d.download(data.dtype, data.size).reshape(data.shape)
        d.free()
        return out

    def free(self):
        for b in (self.d_in, self.d_m, self.d_out):
            b.free()


def same_bits(a, b):
    bits = np.uint64 if a.dtype == np.float64 else np.uint32
    return a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(bits), np.ascontiguousarray(b).view(bits))


def check_independence(c, k, lidar, data, motions, rho, got):
    """the per-point arithmetic depends on (motion, column, rho) only: a scan de-skewed in a call that the launcher splits
    differently gives the same bytes"""
    n, h, w = CASES[k][:3]
    g = capi.deskew_launch_geometry(n, h, w)
    if n > 1:
        other = capi.deskew_launch_geometry(1, h, w)
        for s in uniq([0, n // 3, (2 * n) // 3, n - 1]):
            alone = c.deskew_scans(data[s], lidar, motions[s], rho)
            assert same_bits(alone, got[s]), (case_id(k), rho, s, "alone against the batch")
    else:  # one scan IS the call alone: put it into a batch of three
        other = capi.deskew_launch_geometry(3, h, w)
        three = c.deskew_scans(np.ascontiguousarray(np.repeat(data, 3, axis=0)), lidar, np.repeat(motions, 3, axis=0), rho)
        for s in range(3):
            assert same_bits(three[s], got[0]), (case_id(k), rho, s, "in a batch of three against alone")
    if h > 1:
        assert (other.shares, other.lines_per_share) != (g.shares, g.lines_per_share), (case_id(k), g, other)


@pytest.mark.parametrize("rho", RHOS)
@pytest.mark.parametrize("k", range(len(CASES)), ids=case_id)
def test_every_loop_form_against_numpy(k, rho):
    n, h, w = CASES[k][:3]
    g, form = measured(k)
    assert form == CASES[k][3:] and g.unroll == 4, (case_id(k), "the launcher no longer gives this case its form", g)
    c = ctx()
    lidar = capi.LidarParams(h, w, 1.0, 120.0)
    xyz, motions, special, slots = inputs(k)

    # FP64, out of place between guard bytes, against numpy; in place gives the same bytes
    dev = Dev(c, xyz, motions)
    got = dev.out_of_place(lidar, rho).copy()
    assert same_bits(dev.in_place(lidar, rho), got), (case_id(k), rho, "in place against out of place")
    dev.free()
    live = np.isfinite(xyz).all(axis=2) & ~(xyz == 0).all(axis=2)
    assert (~live).sum() == len(special) and live.sum() + len(special) == n * h * w
    ratio = np.zeros((n, h * w))
    for s in range(n):
        want = deskew_numpy(xyz[s], motions[s], rho, h, w)
        with np.errstate(invalid="ignore"):
            ratio[s] = np.linalg.norm(got[s] - want, axis=1) / bound(xyz[s], motions[s, 4:])
    worst = float(ratio[live].max()) if live.any() else 0.0
    _worst[(case_id(k), rho)] = worst
    print(case_id(k), "rho", rho, "geometry", tuple(g), "worst error / bound()", worst, "pass-through points per slot", slots)
    assert (ratio[live] <= 1.0).all(), (case_id(k), rho, worst, np.argwhere(live & ~(ratio <= 1.0))[:5].tolist())
    assert same_bits(got[~live], xyz[~live]), (case_id(k), rho, "a zero or non-finite point did not come back bit for bit")
    # the neighbours of the pass-through points in line and column (live by construction) are among the points just checked
    grid_live, grid_ratio = live.reshape(n, h, w), ratio.reshape(n, h, w)
    for (s, l, col) in special:
        for dl, dc in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            if 0 <= l + dl < h and 0 <= col + dc < w:
                assert grid_live[s, l + dl, col + dc] and grid_ratio[s, l + dl, col + dc] <= 1.0, (case_id(k), rho, s, l, col, dl, dc)
    check_independence(c, k, lidar, xyz, motions, rho, got)

    # FP32: the FP64 form's result on the widened scans, rounded to float, within one ulp of float per coordinate
    # (criterion (a) of test_gpu_deskew.test_formula_parity)
    b32 = np.ascontiguousarray(xyz.astype(np.float32))
    live32 = np.isfinite(b32).all(axis=2) & ~(b32 == 0).all(axis=2)
    assert np.array_equal(live32, live)
    dev = Dev(c, b32, motions)
    got32 = dev.out_of_place(lidar, rho).copy()
    dev.free()
    assert got32.dtype == np.float32
    dev32 = c.deskew_scans(b32.astype(np.float64), lidar, motions, rho).astype(np.float32)
    ulp = np.spacing(np.abs(dev32[live])).astype(np.float64)
    diff = np.abs(got32[live].astype(np.float64) - dev32[live].astype(np.float64))
    print(case_id(k), "rho", rho, "f32 against the FP64 form rounded: coordinates that differ", int((diff > 0).sum()), "by more than an ulp",
          int((diff > ulp).sum()))
    assert (diff <= ulp).all(), (case_id(k), rho, "f32")
    assert same_bits(got32[~live], b32[~live]), (case_id(k), rho, "f32 pass-through")
    check_independence(c, k, lidar, b32, motions, rho, got32)


def test_the_cases_cover_every_form_of_the_line_loop():
    """from the readout, not from the table: lines per share 1, 2, 3 (the remainder alone), 8 (two full bodies), 5, 9, 10 (bodies and
    a remainder of 1, 1, 2); short last shares; narrow last column blocks; pass-through points in every slot of the loop"""
    forms = [measured(k) for k in range(len(CASES))]
    lps = [f[1] for _, f in forms]
    assert {1, 2, 3, 5, 8, 9, 10} <= set(lps), lps
    short_last = [case_id(k) for k, (_, f) in enumerate(forms) if f[3] < f[1]]
    narrow = [case_id(k) for k, (_, f) in enumerate(forms) if f[4] < BLOCK]
    assert len(short_last) >= 3 and len(narrow) >= 3, (short_last, narrow)
    assert any(f[2] > 1 and f[0] > 1 for _, f in forms)  # (several shares and several column blocks in one grid)
    unroll = forms[0][0].unroll
    count = dict(u0_only=sum(l == 1 for l in lps), remainder_only=sum(1 < l < unroll for l in lps),
                 full_bodies_only=sum(l % unroll == 0 for l in lps), bodies_and_remainder=sum(l > unroll and l % unroll != 0 for l in lps),
                 short_last_share=len(short_last), narrow_last_block=len(narrow))
    for u in (1, 2, 3):  # every slot of the loop holds pass-through points in some case, and the remainder's slots too
        assert sum(placement(k)[1][u] > 0 for k in range(len(CASES))) >= 3, u
    print("cases per loop form:", count)
    assert all(v >= 1 for v in count.values()), count
    if _worst:
        (where, rho), w = max(_worst.items(), key=lambda kv: kv[1])
        print("worst error / bound() over", len(_worst), "runs:", w, "at", where, "rho", rho)
