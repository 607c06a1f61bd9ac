"""The rule of the map cleaning (include/loamx.h, "map cleaning") in plain numpy: the map point into the sensor frame, its cell
from organize_common.classify on the layout's two tables, the range band, the window over the scan, the verdict, the votes and
the decision. float64 operations one at a time in the header's order (numpy's elementwise loops round every operation on its
own), so everything is compared by equality. It carries its own restatement of the inverse pose. No code shared with the
kernels. Also: the drive with a moving box the tests share, and the binding of tests/hostcheck_visibility."""
import ctypes as C
import os
import subprocess

import numpy as np

import cloudmap_common as CM
import organize_common as O
import outdoor_scenes as S

THROUGH, AGREE, OCCLUDED, EMPTY, NONE = range(5)
VOTES_DTYPE = np.dtype([("through", np.uint32), ("agree", np.uint32), ("occluded", np.uint32), ("empty", np.uint32)])
FIELDS = VOTES_DTYPE.names
SCAN_CHUNK = 32  # scans per workgroup row of the votes kernel (include/loamx.h)


class Params:
    """loamx_visibility_params with the header's defaults"""
    DEFAULTS = dict(min_range=1.0, max_range=80.0, margin=0.3, margin_rel=0.01, window_lines=1, window_cols=1, min_through=2, through_ratio=1.0)

    def __init__(self, **kw):
        for k, v in self.DEFAULTS.items():
            setattr(self, k, kw.pop(k, v))
        assert not kw, kw

    def items(self):
        return {k: getattr(self, k) for k in self.DEFAULTS}


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def to_sensor(points, pose):
    """step 1 on (n, 3) world points: d = m - t, p = d + qw (2 u x d) + u x (2 u x d) with u = (-qx, -qy, -qz)"""
    pose = np.asarray(pose, dtype=np.float64)
    with np.errstate(all="ignore"):
        d = tuple(points[:, k] - pose[4 + k] for k in range(3))
        u = (-pose[0], -pose[1], -pose[2])
        uv = _cross(u, d)
        uv = tuple(c + c for c in uv)
        cc = _cross(u, uv)
        return np.stack([(d[k] + pose[3] * uv[k]) + cc[k] for k in range(3)], axis=1)


def cell_r2(scan, min2):
    """step 5's r2c per cell of one scan (H W, 3), any float dtype, and which cells are usable"""
    s = np.asarray(scan).reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        r2c = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
        usable = np.isfinite(s).all(axis=1) & (r2c >= min2)
    return r2c, usable


def bounds(r2, p):
    """step 4: (lo2, hi2)"""
    with np.errstate(all="ignore"):
        dist = np.sqrt(r2)
        tol = p.margin + p.margin_rel * dist
        lo = dist - tol
        lo = np.where(lo < 0.0, 0.0, lo)
        hi = dist + tol
        return lo * lo, hi * hi


def verdicts(points, scan, pose, H, W, col_dirs, line_tans, clockwise=False, params=None):
    """per map point (n, >= 3) its verdict in one scan, and how far it came: 0 none, 1 in range (step 2), 2 projected (step 3)"""
    p = params or Params()
    m = np.asarray(points, dtype=np.float64)[:, :3]
    n = len(m)
    verdict, place = np.full(n, NONE, dtype=np.int64), np.zeros(n, dtype=np.int64)
    if n == 0:
        return verdict, place
    min2, max2 = p.min_range * p.min_range, p.max_range * p.max_range
    q = to_sensor(m, pose)
    with np.errstate(all="ignore"):
        rho2 = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]
        r2 = rho2 + q[:, 2] * q[:, 2]
        valid = np.isfinite(q).all(axis=1) & np.isfinite(r2) & (rho2 >= 1e-100)
        in_range = valid & (r2 >= min2) & (r2 <= max2)
    idx = np.flatnonzero(in_range)
    place[idx] = 1
    if not len(idx):
        return verdict, place
    cell, r2c_pts = O.classify(q[idx], col_dirs, line_tans, clockwise)
    assert np.array_equal(r2c_pts.view(np.uint64), r2[idx].view(np.uint64)) and not (cell == O.INVALID).any()
    proj = cell != O.OUTSIDE
    idx, cell = idx[proj], cell[proj].astype(np.int64)
    place[idx] = 2
    if not len(idx):
        return verdict, place
    line, col = cell // W, cell % W
    lo2, hi2 = bounds(r2[idx], p)
    r2c, usable = cell_r2(scan, min2)
    any_usable, any_agree, all_beyond = np.zeros(len(idx), bool), np.zeros(len(idx), bool), np.ones(len(idx), bool)
    for dl in range(-int(p.window_lines), int(p.window_lines) + 1):
        ll = line + dl
        ok_line = (ll >= 0) & (ll < H)
        for dc in range(-int(p.window_cols), int(p.window_cols) + 1):
            c = np.where(ok_line, ll, 0) * W + (col + dc) % W
            use = ok_line & usable[c]
            r = r2c[c]
            any_usable |= use
            any_agree |= use & (r >= lo2) & (r <= hi2)
            all_beyond &= ~use | (r > hi2)
    verdict[idx] = np.where(~any_usable, EMPTY, np.where(any_agree, AGREE, np.where(all_beyond, THROUGH, OCCLUDED)))
    return verdict, place


def votes_per_point(points, scans, poses, H, W, col_dirs, line_tans, clockwise=False, params=None, into=None):
    """(votes (n,) VOTES_DTYPE, per point the scans in whose range band it lay, per point the scans in which it had a cell) over
    scans (n_scans, H W, 3) at poses (n_scans, 7); into: votes to add to"""
    n = len(points)
    out = np.zeros(n, dtype=VOTES_DTYPE) if into is None else into.copy()
    in_range, projected = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for s in range(len(scans)):
        v, place = verdicts(points, scans[s], poses[s], H, W, col_dirs, line_tans, clockwise, params)
        for k, name in enumerate(FIELDS):
            out[name] += (v == k).astype(np.uint32)
        in_range += place >= 1
        projected += place == 2
    return out, in_range, projected


def votes(points, scans, poses, H, W, col_dirs, line_tans, clockwise=False, params=None, into=None):
    """(votes, in-range pairs, projected pairs): votes_per_point with the two census counts summed"""
    out, in_range, projected = votes_per_point(points, scans, poses, H, W, col_dirs, line_tans, clockwise, params, into)
    return out, int(in_range.sum()), int(projected.sum())


def dynamic(v, params=None):
    """the decision per point: through >= min_through and (double) through >= through_ratio (double) agree"""
    p = params or Params()
    with np.errstate(all="ignore"):
        need = np.float64(p.through_ratio) * v["agree"].astype(np.float64)
        return (v["through"] >= np.uint32(p.min_through)) & (v["through"].astype(np.float64) >= need)


def filter_static(v, params=None, points=None, capacity=None):
    """(dynamic (n,) uint8, kept xyz or None, kept indices uint32, n kept) as loamx_visibility_filter_dev: kept points in input order"""
    dyn = dynamic(v, params)
    keep = np.flatnonzero(~dyn).astype(np.uint32)
    n = len(keep)
    keep = keep if capacity is None else keep[:capacity]
    xyz = None if points is None else np.ascontiguousarray(np.asarray(points, dtype=np.float64)[keep, :3])
    return dyn.astype(np.uint8), xyz, keep, n


def same_bytes(a, b):
    return CM.same_bytes(a, b)


def analytic_tables(H, W, fan_deg):
    """(col_dirs, line_tans) of a counter-clockwise layout with azimuth_zero 0 and the beam elevations of outdoor_scenes for a fan,
    by the header's formulas in numpy (the CPU tests' stand-in for loamx_scan_layout_tables; the GPU tests read the library's)"""
    el = O.fan_elevations(H, fan_deg)
    phi = 2.0 * np.pi * (np.arange(W) - 0.5) / W
    b = np.concatenate([[el[0] - (el[1] - el[0]) / 2.0], (el[:-1] + el[1:]) / 2.0, [el[-1] + (el[-1] - el[-2]) / 2.0]])
    return np.stack([np.cos(phi), np.sin(phi)], axis=1), np.tan(b)


# ---- inputs the tests share ------------------------------------------------------------------------------------------------------
def shell_scan(rng, H, W, fan=(15.0, -15.0), radius=20.0, spread=3.0, holes=True, dtype=np.float64):
    """a scan whose cell (l, c) looks along the cell's own direction and returns from radius +- spread; with holes: zero cells,
    NaN and inf cells, and cells nearer than a min_range of 1"""
    el = O.fan_elevations(H, fan) if H > 1 else np.zeros(1)
    az = 2.0 * np.pi * np.arange(W) / W
    r = radius + rng.uniform(-spread, spread, (H, W))
    d = np.stack([np.cos(el)[:, None] * np.cos(az)[None, :], np.cos(el)[:, None] * np.sin(az)[None, :], np.broadcast_to(np.sin(el)[:, None], (H, W))], -1)
    scan = (d * r[..., None]).reshape(-1, 3)
    if holes:
        kind = rng.random(H * W)
        scan[kind < 0.06] = 0.0
        scan[(kind >= 0.06) & (kind < 0.09), 1] = np.nan
        scan[(kind >= 0.09) & (kind < 0.11), 2] = np.inf
        scan[(kind >= 0.11) & (kind < 0.14)] *= 0.02  # nearer than min_range
    return np.ascontiguousarray(scan.astype(dtype))


def cloud(rng, n, lo=0.3, hi=35.0, el=(-0.5, 0.5)):
    """n points in a shell around the origin, elevations beyond a 15 degree fan on both sides"""
    az, e, r = rng.uniform(0, 2 * np.pi, n), rng.uniform(*el, n), rng.uniform(lo, hi, n)
    return np.stack([r * np.cos(e) * np.cos(az), r * np.cos(e) * np.sin(az), r * np.sin(e)], 1)


# ---- the drive with a moving box ------------------------------------------------------------------------------------------------
BOX_SIZE = (4.4, 1.8, 1.6)


def drive(H=16, W=256, n_scans=16, leaf=0.4, seed=0, step=1.0, box_step=1.5, dtype=np.float32):
    """n_scans scans of the lot scene from a sensor that drives along +x, with a box of BOX_SIZE that comes towards it by box_step
    per scan in the next lane. Returns a dict: scans (n, H W, 3) dtype, poses (n, 7), points (the voxel centroids of all scans at
    `leaf`, in the cloud map's order), is_box / is_static (per voxel: all / none of its points are returns from the box)."""
    boxes = S.scene_boxes("lot", seed)
    o0 = np.array([-7.0, 0.0, S.SENSOR_HEIGHT])
    lx, ly, lz = BOX_SIZE
    scans, poses, world, hit_box = [], [], [], []
    for i in range(n_scans):
        origin = o0 + np.array([step * i, 0.0, 0.0])
        cx = 26.0 - box_step * i
        box = S._box(cx - lx / 2, cx + lx / 2, 3.0 - ly / 2, 3.0 + ly / 2, 0.0, lz)
        with_box = S.cast(boxes + [box], origin, 0.0, H, W, S.FANS["lot"], 0.01, np.random.default_rng([seed, i]))
        without = S.cast(boxes, origin, 0.0, H, W, S.FANS["lot"], 0.01, np.random.default_rng([seed, i]))
        scan = with_box.astype(dtype)
        scans.append(scan)
        poses.append(S.yaw_pose(0.0, origin))
        hit_box.append((with_box != without).any(axis=1))
        world.append(CM.pose_act(poses[-1], scan.astype(np.float64)))
    scans, poses, hit_box = np.ascontiguousarray(scans), np.ascontiguousarray(poses), np.concatenate(hit_box)
    model = CM.CloudMapModel(leaf, 0.5, 120.0)
    model.add(scans.reshape(-1, 3), np.arange(n_scans + 1) * (H * W), poses)
    points = model.emit()[0]
    # which voxel every used point went into, by the cloud map's own cell rule
    flat = scans.reshape(-1, 3).astype(np.float64)
    used = CM.validity(flat, 0.5, 120.0) == CM.USED
    ok, v, _ = CM.cells(np.concatenate(world), leaf)
    used &= ok
    order = {k: j for j, k in enumerate(model.vox.keys())}
    slot = np.array([order[int(k)] for k in CM.pack(v[used])], dtype=np.int64)
    n_box = np.bincount(slot, weights=hit_box[used].astype(np.float64), minlength=len(points))
    n_all = np.bincount(slot, minlength=len(points))
    assert (n_all > 0).all()
    return dict(scans=scans, poses=poses, points=np.ascontiguousarray(points), is_box=n_box == n_all, is_static=n_box == 0, H=H, W=W, leaf=leaf)


# ---- tests/hostcheck_visibility: visibility_math.h compiled by g++ ---------------------------------------------------------------
HOSTCHECK_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck_visibility")
_lib = None


def hostcheck_lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", HOSTCHECK_DIR])
        _lib = C.CDLL(os.path.join(HOSTCHECK_DIR, "libhostcheck_visibility.so"))
    return _lib


def header_verdicts(points, scan, pose, H, W, col_dirs, line_tans, clockwise=False, params=None):
    """visibility_math.h under g++ for one scan (float64 or float32): (verdict, place) per point as verdicts()"""
    p = params or Params()
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64)[:, :3])
    scan = np.ascontiguousarray(scan)
    assert scan.dtype in (np.float32, np.float64) and scan.size == H * W * 3
    col = np.ascontiguousarray(col_dirs, dtype=np.float64)
    tan = np.ascontiguousarray(line_tans, dtype=np.float64)
    pose = np.ascontiguousarray(pose, dtype=np.float64)
    verdict, place = np.zeros(len(pts), dtype=np.int32), np.zeros(len(pts), dtype=np.int32)
    rule = (C.c_double * 4)(p.min_range * p.min_range, p.max_range * p.max_range, p.margin, p.margin_rel)
    dp = C.POINTER(C.c_double)
    hostcheck_lib().hostcheck_visibility_verdicts(
        pts.ctypes.data_as(dp), C.c_uint64(len(pts)), C.c_void_p(scan.ctypes.data), C.c_int(scan.dtype == np.float32), pose.ctypes.data_as(dp),
        C.c_uint32(H), C.c_uint32(W), col.ctypes.data_as(dp), tan.ctypes.data_as(dp), C.c_uint32(1 if clockwise else 0), rule,
        C.c_uint32(p.window_lines), C.c_uint32(p.window_cols), verdict.ctypes.data_as(C.POINTER(C.c_int32)), place.ctypes.data_as(C.POINTER(C.c_int32)))
    return verdict.astype(np.int64), place.astype(np.int64)


def header_dynamic(v, params=None):
    p = params or Params()
    v = np.ascontiguousarray(v)
    out = np.zeros(len(v), dtype=np.uint8)
    hostcheck_lib().hostcheck_visibility_dynamic(C.c_void_p(v.ctypes.data), C.c_uint64(len(v)), C.c_uint32(p.min_through), C.c_double(p.through_ratio),
                                                 out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return out.astype(bool)
