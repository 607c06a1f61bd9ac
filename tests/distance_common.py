"""The rule of the occupancy distance field (include/loamx.h, "occupancy distance field") in plain numpy: which voxels are
obstacles (from the states of tests/occupancy_common.py's OccupancyModel), and per voxel of a box or column of a slice the squared
distance to the nearest obstacle, the offset to it and the metres. The field is a BRUTE-FORCE search: every obstacle within the
halo is a candidate, the candidates stand in linear order (z, then y, then x) and argmin takes the first of equal minima, which is
the minimiser with the lowest linear index. No separable passes and no code shared with the kernels. Everything is integer but
the metres, so everything is compared by equality. scipy.ndimage.distance_transform_edt is an independent check of d2
(edt_d2). Also: the named cases both the g++ build and the kernels are compared on, and the binding of tests/hostcheck_distance."""
import os
import subprocess
import tempfile

import numpy as np

import occupancy_common as M

FAR = 0xFFFF
same_bytes = M.same_bytes


# ---- the field of a list of obstacles ---------------------------------------------------------------------------------------------
def field(obstacles, vmin, dims, R, leaf=0.2):
    """obstacles: (m, A) integer voxel coordinates (A = 3, or 2 for a slice's columns), anywhere on the lattice; vmin, dims: the
    first A entries are used. -> (d2 dims[::-1] uint16, offset dims[::-1] + (A,) int16, metres float32)"""
    obstacles = np.asarray(obstacles, dtype=np.int64)
    A = obstacles.shape[1] if obstacles.ndim == 2 else len(vmin)
    obstacles = obstacles.reshape(-1, A)
    vmin, dims = np.asarray(vmin, dtype=np.int64)[:A], np.asarray(dims, dtype=np.int64)[:A]
    shape = tuple(int(d) for d in dims[::-1])
    n = int(np.prod(dims))
    d2 = np.full(n, FAR, dtype=np.uint16)
    offset = np.zeros((n, A), dtype=np.int16)
    # the candidates: inside the halo, in linear order (the last axis slowest)
    near = np.all((obstacles >= vmin - R) & (obstacles <= vmin + dims - 1 + R), axis=1)
    cand = np.unique(obstacles[near], axis=0) if near.any() else obstacles[:0]
    if len(cand):
        cand = cand[np.lexsort([cand[:, a] for a in range(A)])]  # (the last key is the primary one: z, then y, then x)
    if n and len(cand):
        grids = np.meshgrid(*[np.arange(int(d)) for d in dims[::-1]], indexing="ij")  # z, y, x
        vox = np.stack([g.ravel() for g in grids[::-1]], axis=1) + vmin  # (n, A) in x, y, z order, x fastest
        step = max(1, (1 << 22) // len(cand))
        for i0 in range(0, n, step):
            v = vox[i0:i0 + step]
            diff = cand[None, :, :] - v[:, None, :]
            dist = (diff * diff).sum(axis=2)
            first = np.argmin(dist, axis=1)  # the first of equal minima
            best = dist[np.arange(len(v)), first]
            ok = best <= R * R
            d2[i0:i0 + step][ok] = best[ok].astype(np.uint16)
            offset[i0:i0 + step][ok] = diff[np.arange(len(v)), first][ok].astype(np.int16)
    return d2.reshape(shape), offset.reshape(shape + (A,)), metres_of(d2, leaf).reshape(shape)


def metres_of(d2, leaf):
    """(float)(sqrt((double) d2) * leaf), +inf for FAR"""
    d2 = np.asarray(d2)
    with np.errstate(all="ignore"):
        m = (np.sqrt(d2.astype(np.float64)) * np.float64(leaf)).astype(np.float32)
    return np.where(d2 == FAR, np.float32(np.inf), m).astype(np.float32)


def edt_d2(obstacles, vmin, dims, R):
    """the independent check: rint(edt^2) of scipy's exact Euclidean transform on the extended box, cut back to the box; only
    meaningful where it is <= R^2 (beyond that an obstacle outside the extended box could be nearer)"""
    from scipy.ndimage import distance_transform_edt
    obstacles = np.asarray(obstacles, dtype=np.int64)
    A = obstacles.shape[1]
    vmin, dims = np.asarray(vmin, dtype=np.int64)[:A], np.asarray(dims, dtype=np.int64)[:A]
    emin, edims = vmin - R, dims + 2 * R
    free = np.ones(tuple(int(d) for d in edims[::-1]), dtype=bool)
    c = obstacles - emin
    inside = np.all((c >= 0) & (c < edims), axis=1)
    free[tuple(c[inside, a] for a in range(A - 1, -1, -1))] = False
    if free.all():
        return np.full(tuple(int(d) for d in dims[::-1]), np.inf)
    e = distance_transform_edt(free)
    e2 = np.rint(e * e)
    return e2[tuple(slice(R, R + int(d)) for d in dims[::-1])]


# ---- the obstacles of an occupancy model --------------------------------------------------------------------------------------
def obstacles_of(model, vmin, dims, R, unknown_is_obstacle=False, slice2d=False):
    """the obstacle voxels (m, 3), or columns (m, 2), that can matter to the box. Without unknown_is_obstacle (and with thresholds
    under which a voxel without counts is not OCCUPIED) they come from the model's OCCUPIED voxels, so a large R costs nothing;
    otherwise from the states of the dense extended box."""
    vmin, dims = np.asarray(vmin, dtype=np.int64), np.asarray(dims, dtype=np.int64)
    p = model.p
    empty_state = int(M.state(0, 0, p["min_hits"], p["occ_ratio"], p["min_passes"]))
    if not unknown_is_obstacle and empty_state != M.OCCUPIED:
        if not model.vox:
            return np.zeros((0, 2 if slice2d else 3), dtype=np.int64)
        keys = list(model.vox)
        counts = np.array([model.vox[k] for k in keys], dtype=np.uint32)
        occ = M.key_coords(keys)[model._state(counts) == M.OCCUPIED]
        if not slice2d:
            return occ
        in_levels = (occ[:, 2] >= vmin[2]) & (occ[:, 2] < vmin[2] + dims[2])
        return np.unique(occ[in_levels, :2], axis=0) if in_levels.any() else occ[:0, :2]
    emin, edims = vmin - R, dims + 2 * R
    if slice2d:
        emin[2], edims[2] = vmin[2], dims[2]
        st = model.slice(emin, edims)  # (ey, ex)
    else:
        st = model.box(emin, edims)[1]  # (ez, ey, ex)
    obstacle = (st == M.OCCUPIED) | ((st == M.UNKNOWN) if unknown_is_obstacle else False)
    idx = np.argwhere(obstacle)[:, ::-1]  # x, y(, z)
    return idx + emin[:idx.shape[1]]


def model_field(model, vmin, dims, R, unknown_is_obstacle=False, slice2d=False):
    obst = obstacles_of(model, vmin, dims, R, unknown_is_obstacle, slice2d)
    return field(obst, vmin, dims, R, model.p["leaf"])


# ---- placing obstacles in a map: one ray per obstacle that stays inside its voxel ----------------------------------------------------
PLACE = dict(min_range=0.01, end_margin=0.0)  # the thresholds under which place_rays leaves exactly one hit and no pass per voxel


def place_rays(voxels, leaf):
    """(points (m, 3), offsets, poses (m, 7)): one cloud of one ray per voxel. The sensor stands at the voxel's centre and the
    return 0.2 leaf further along x: hit and walk lie in the voxel, whose own hit voxel takes no pass."""
    voxels = np.asarray(voxels, dtype=np.int64).reshape(-1, 3)
    m = len(voxels)
    pts = np.tile([0.2 * leaf, 0.0, 0.0], (m, 1))
    poses = np.zeros((m, 7))
    poses[:, 3] = 1.0
    poses[:, 4:] = (voxels + 0.5) * leaf
    return pts, np.arange(m + 1, dtype=np.uint64), poses


# ---- the named cases (no table needed: a list of obstacle voxels, a box, R) ---------------------------------------------------------
def named_cases():
    """name -> dict(obst (m, 3), vmin, dims, R); `slice` marks 2-D cases (the z of the obstacles is vmin[2]).
    The field of each is asserted where it is the point of the case (test_distance_hostcheck.py)."""
    c = {}

    def case(name, obst, vmin, dims, R, **kw):
        c[name] = dict(obst=np.asarray(obst, dtype=np.int64).reshape(-1, 3), vmin=np.asarray(vmin, dtype=np.int64),
                       dims=np.asarray(dims, dtype=np.int64), R=R, **kw)

    # mask words: extended x lengths 63, 64, 65 and 129 (dims[0] + 2R), obstacles at both ends of the rows and in the middle
    for ex in (63, 64, 65, 129):
        R = 3
        dx = ex - 2 * R
        obst = [(-R, 0, 0), (dx - 1 + R, 1, 0), (dx // 2, 0, 1), (0, -R, -R), (dx - 1, 1 + R, 1 + R), (dx - 2, 0, 0)]
        case(f"mask_words_ex_{ex}", obst, (0, 0, 0), (dx, 2, 2), R)
    # a window that spans three words: R = 70
    case("window_of_three_words", [(-70, 0, 0), (72, 1, 1), (1, 0, 60)], (0, 0, 0), (3, 2, 2), 70)
    case("window_of_three_words_far", [(-71, 0, 0), (73, 1, 1)], (0, 0, 0), (3, 2, 2), 70)
    # an obstacle in the last bit of one word, the voxel in the first bit of the next (R = 4: position = x + 4)
    case("last_bit_then_first_bit", [(59, 0, 0), (123, 1, 0)], (56, 0, 0), (70, 2, 1), 4)
    # the cap
    case("cap_25_reported", [(3, 4, 0)], (0, 0, 0), (1, 1, 1), 5)
    case("cap_26_far", [(3, 4, 1)], (0, 0, 0), (1, 1, 1), 5)
    case("cap_65025_reported", [(180, 180, 15)], (0, 0, 0), (2, 1, 1), 255)
    case("cap_65026_far", [(180, 180, 19)], (0, 0, 0), (2, 1, 1), 255)
    for a in range(3):
        for d in (255, 256):
            for s in (1, -1):
                w = [0, 0, 0]
                w[a] = s * d
                case(f"cap_axis_{a}_{'plus' if s > 0 else 'minus'}_{d}", [tuple(w)], (0, 0, 0), (2, 1, 1), 255)
    # ties: +-d on one, two and three axes, the eight corners of a cube
    v = (2, 2, 2)
    for d in (1, 3):
        for axes in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)):
            obst = []
            for a in axes:
                for s in (1, -1):
                    w = list(v)
                    w[a] += s * d
                    obst.append(tuple(w))
            case(f"ties_pm{d}_axes_{''.join(map(str, axes))}", obst, (0, 0, 0), (5, 5, 5), 4)
        corners = [(v[0] + sx * d, v[1] + sy * d, v[2] + sz * d) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
        case(f"ties_cube_corners_{d}", corners, (0, 0, 0), (5, 5, 5), 6)
    # the stop rule's edge: the best so far is k^2 (from an intermediate off the axis) and a candidate with a ZERO intermediate sits
    # exactly k away, on the lower side (it wins the tie) and on the higher side (it does not)
    case("stop_edge_lower_y", [(5, 3, 3), (3, 1, 3)], (3, 3, 3), (1, 1, 1), 4)   # dx = 2 at y' = y: 4; y' = y - 2, dx = 0: 4 -> the lower y
    case("stop_edge_higher_y", [(1, 3, 3), (3, 5, 3)], (3, 3, 3), (1, 1, 1), 4)  # y' = y + 2 ties and loses
    case("stop_edge_lower_z", [(3, 5, 3), (3, 3, 1)], (3, 3, 3), (1, 1, 1), 4)
    case("stop_edge_higher_z", [(3, 1, 3), (3, 3, 5)], (3, 3, 3), (1, 1, 1), 4)
    case("stop_edge_3_4_5", [(3, 4, 0), (0, 0, 5), (0, 0, -5), (5, 0, 0), (-5, 0, 0), (0, -5, 0)], (0, 0, 0), (1, 1, 1), 5)
    # halo: seen at R outside the box, not at R + 1; boxes with dims of 1; negative vmin
    R = 3
    for a in range(3):
        dims = [4, 3, 2]
        for s, tag in ((1, "above"), (-1, "below")):
            for extra in (0, 1):
                w = [1, 1, 1]
                w[a] = (dims[a] - 1 + R + extra) if s > 0 else -(R + extra)
                vmin = np.array([-7, -20, -3])
                case(f"halo_axis_{a}_{tag}_{'R_plus_1' if extra else 'R'}", [tuple(np.array(w) + vmin)], vmin, dims, R)
    for dims in ((1, 4, 3), (4, 1, 3), (4, 3, 1), (1, 1, 1)):
        case(f"dims_of_one_{'x'.join(map(str, dims))}", [(-1, -2, -9), (-3, 0, -8), (-2, -1, -13)], (-3, -2, -10), dims, 3)
    # empty map
    case("no_obstacles", np.zeros((0, 3)), (-2, -2, -2), (5, 4, 3), 4)
    # 2-D
    case("slice_ties", [(2, 0, 0), (0, 2, 0), (4, 2, 0), (2, 4, 0)], (0, 0, 0), (5, 5, 1), 3, slice=True)
    case("slice_cap", [(3, 4, 0), (-6, 0, 0)], (0, 0, 0), (2, 1, 1), 5, slice=True)
    case("slice_ex_65", [(-2, 0, 0), (62, 1, 0), (30, 3, 0)], (0, 0, 0), (61, 2, 1), 2, slice=True)
    return c


def case_field(case, leaf=0.2):
    A = 2 if case.get("slice") else 3
    return field(case["obst"][:, :A], case["vmin"], case["dims"], case["R"], leaf)


def random_boxes(n=200, seed=7):
    """n random boxes with R in 1 .. 7 and obstacle densities 0, 0.5 %, 3 %, 20 % in the extended box; every fifth is a slice"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        R = int(rng.integers(1, 8))
        dims = rng.integers(1, 10, 3)
        if i % 7 == 0:
            dims[0] = int(rng.choice([64 - 2 * R, 65 - 2 * R, 130 - 2 * R]))  # rows of one, two and three mask words
        vmin = rng.integers(-50, 50, 3)
        density = (0.0, 0.005, 0.03, 0.2)[i % 4]
        is_slice = i % 5 == 4
        edims = dims + 2 * R
        if is_slice:
            edims[2] = 1
        mask = rng.uniform(size=tuple(edims[::-1])) < density
        obst = np.argwhere(mask)[:, ::-1] + (vmin - R)
        if is_slice:
            obst[:, 2] = vmin[2]
            dims[2] = 1
        out.append(dict(obst=obst.astype(np.int64), vmin=vmin.astype(np.int64), dims=dims.astype(np.int64), R=R, slice=is_slice))
    return out


# ---- tests/hostcheck_distance: distance_math.h compiled by g++ ------------------------------------------------------------------------
HOSTCHECK_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck_distance")
HEADER = np.dtype([("dims", np.uint32, 3), ("R", np.uint32), ("slice", np.uint32), ("early", np.uint32), ("n_obstacles", np.uint32),
                   ("pad", np.uint32), ("leaf", np.float64)])
assert HEADER.itemsize == 40


def hostcheck_program(san=False):
    subprocess.check_call(["make", "-s", "-C", HOSTCHECK_DIR] + (["san"] if san else []))
    return os.path.join(HOSTCHECK_DIR, "hostcheck_distance_san" if san else "hostcheck_distance")


def hostcheck_run(program, cases, early, leaf=0.2):
    """[(d2, offset, metres)] per case, shaped as field()'s"""
    blobs, shapes = [], []
    for c in cases:
        is_slice = bool(c.get("slice"))
        R, dims, vmin = int(c["R"]), np.asarray(c["dims"], dtype=np.int64).copy(), np.asarray(c["vmin"], dtype=np.int64)
        emin, edims = vmin - R, dims + 2 * R
        obst = np.asarray(c["obst"], dtype=np.int64).reshape(-1, 3).copy()
        if is_slice:
            obst[:, 2], emin[2], edims[2], dims[2] = 0, 0, 1, 1
        pos = obst - emin
        pos = pos[np.all((pos >= 0) & (pos < edims), axis=1)]
        h = np.zeros(1, dtype=HEADER)
        h["dims"], h["R"], h["slice"], h["early"], h["n_obstacles"], h["leaf"] = dims, R, int(is_slice), int(early), len(pos), leaf
        blobs += [h.tobytes(), np.ascontiguousarray(pos, dtype=np.uint32).tobytes()]
        shapes.append(((int(dims[1]), int(dims[0])) if is_slice else (int(dims[2]), int(dims[1]), int(dims[0])), 2 if is_slice else 3))
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(b"".join(blobs))
        r = subprocess.run([program, fin, fout], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        raw = open(fout, "rb").read()
    out, at = [], 0
    for shape, axes in shapes:
        n = int(np.prod(shape))
        d2 = np.frombuffer(raw, np.uint16, n, at).reshape(shape)
        at += 2 * n
        off = np.frombuffer(raw, np.int16, n * axes, at).reshape(shape + (axes,))
        at += 2 * n * axes
        m = np.frombuffer(raw, np.float32, n, at).reshape(shape)
        at += 4 * n
        out.append((d2, off, m))
    assert at == len(raw)
    return out
