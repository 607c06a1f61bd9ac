"""The scan segmentation's rule (include/loamx.h, "scan segmentation") restated in numpy, and the scenes its tests share.

Every product, sum and difference is one float64 numpy operation in the order the rule writes them, so the model's predicates
are the kernels' bit for bit; the components come from scipy.sparse.csgraph.connected_components and every other quantity is an
integer. tg2 and c2 are taken from capi.segment_constants (the launcher's own numbers)."""
import collections

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from loam_amd import capi

NO_LABEL = 0xFFFFFFFF
Segmentation = collections.namedtuple("Segmentation", "classes labels sizes filtered clusters stats right up")


def valid_cells(p, min_range, max_range):
    """p: (..., 3) float64"""
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    with np.errstate(all="ignore"):
        r = np.sqrt(x * x + y * y + z * z)
        return np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & ~((r < min_range) | (r > max_range))


def ground_pair(a, b, tg2):
    """a = p(l, c), b = p(l + 1, c): (..., 3) each"""
    with np.errstate(all="ignore"):
        dx, dy, dz = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1], b[..., 2] - a[..., 2]
        return dz * dz <= tg2 * (dx * dx + dy * dy)


def connected(a, b, c2):
    with np.errstate(all="ignore"):
        r2a = (a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]
        r2b = (b[..., 0] * b[..., 0] + b[..., 1] * b[..., 1]) + b[..., 2] * b[..., 2]
        m = np.where(r2a > r2b, r2a, r2b)
        dot = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
        ex, ey, ez = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1], b[..., 2] - a[..., 2]
        e2 = (ex * ex + ey * ey) + ez * ez
        t = m - dot
        return t * t < (c2 * m) * e2


def segment(scan, H, W, min_range=1.0, max_range=120.0, params=None, max_clusters=None):
    """The model. scan: (H W, 3) float64 or float32 (widened first; the filtered scan keeps the dtype). Returns a Segmentation;
    right / up: (H, W) bool, the connected right and up edges per cell (for the census)."""
    params = params or capi.SegmentParams()
    tg2, c2 = capi.segment_constants(params)
    raw = np.asarray(scan).reshape(H, W, 3)
    p = raw.astype(np.float64)
    HW = H * W
    valid = valid_cells(p, min_range, max_range)
    G = int(params.ground_lines)
    G = H if G == 0 or G > H else G
    ground = np.zeros((H, W), bool)
    if G >= 2:
        pair = valid[:G - 1] & valid[1:G] & ground_pair(p[:G - 1], p[1:G], tg2)
        ground[:G - 1] |= pair
        ground[1:G] |= pair
    node = valid & ~ground
    right = np.zeros((H, W), bool)
    if W > 1:
        q = np.roll(p, -1, axis=1)
        right = node & np.roll(node, -1, axis=1) & connected(p, q, c2)
    up = np.zeros((H, W), bool)
    if H > 1:
        up[:-1] = node[:-1] & node[1:] & connected(p[:-1], p[1:], c2)
    idx = np.arange(HW).reshape(H, W)
    src = np.concatenate([idx[right], idx[:-1][up[:-1]]])
    dst = np.concatenate([np.roll(idx, -1, axis=1)[right], idx[1:][up[:-1]]])
    _, comp = connected_components(coo_matrix((np.ones(len(src), np.int8), (src, dst)), shape=(HW, HW)), directed=False)
    flat_node = node.reshape(-1)
    # root of a component = its smallest linear index
    root_of = np.full(comp.max() + 1, HW, np.int64)
    np.minimum.at(root_of, comp, np.arange(HW))
    size_of = np.bincount(comp, minlength=comp.max() + 1)
    line = np.arange(HW) // W
    lmax_of = np.zeros(comp.max() + 1, np.int64)
    np.maximum.at(lmax_of, comp, line)
    lmin_of = root_of // W
    span_of = lmax_of - lmin_of + 1
    acc_of = (size_of >= int(params.min_cluster_points)) | ((size_of >= int(params.min_tall_cluster_points)) & (span_of >= int(params.min_tall_cluster_lines)))
    classes = np.zeros(HW, np.uint8)
    classes[ground.reshape(-1)] = capi.SEGMENT_GROUND
    classes[flat_node] = np.where(acc_of[comp[flat_node]], capi.SEGMENT_CLUSTER, capi.SEGMENT_OUTLIER)
    labels = np.where(flat_node, root_of[comp], NO_LABEL).astype(np.uint32)
    sizes = np.where(flat_node, size_of[comp], 0).astype(np.uint32)
    keep = classes == capi.SEGMENT_CLUSTER
    if not params.drop_outliers:
        keep |= classes == capi.SEGMENT_OUTLIER
    if not params.drop_ground:
        keep |= classes == capi.SEGMENT_GROUND
    filtered = np.where(keep[:, None], raw.reshape(HW, 3), raw.dtype.type(0))
    node_comps = np.unique(comp[flat_node])
    accepted = node_comps[acc_of[node_comps]]
    accepted = accepted[np.argsort(root_of[accepted])]
    clusters = np.zeros(len(accepted), capi.SEGMENT_CLUSTER_DTYPE)
    clusters["root"], clusters["size"] = root_of[accepted], size_of[accepted]
    clusters["line_min"], clusters["line_max"] = lmin_of[accepted], lmax_of[accepted]
    written = len(clusters) if max_clusters is None else min(len(clusters), max_clusters)
    stats = np.array([np.count_nonzero(classes == k) for k in range(4)] +
                     [len(accepted), len(node_comps) - len(accepted), size_of[node_comps].max() if len(node_comps) else 0, written], np.uint32)
    return Segmentation(classes, labels, sizes, np.ascontiguousarray(filtered), clusters[:written], stats, right, up)


def merged_edges(seg, tile_lines, tile_cols, tiles):
    """What loamx_ctx_last_segment_census counts for one scan: the connected edges handed to the global union, per cell and
    direction. Tile form: up edges from the last line of a tile, right edges from the last column of a tile or from column W - 1."""
    H, W = seg.right.shape
    if not tiles:
        return int(seg.right.sum() + seg.up.sum())
    col, lin = np.arange(W), np.arange(H)
    r_out = ((col + 1) % tile_cols == 0) | (col == W - 1)
    u_out = (lin + 1) % tile_lines == 0
    return int(seg.right[:, r_out].sum() + seg.up[u_out].sum())


# ---- mask-drawn scenes: a boolean H x W mask on two concentric spheres ----------------------------------------------------------
def mask_scan(mask, far=20.0, near=10.0, line_gap_deg=2.0):
    """Cells where the mask is set at `near` metres, the others at `far` metres, or (0, 0, 0) where far is None. Azimuth 2 pi c / W,
    lines line_gap_deg apart around the horizon. Under the default 60 degrees and with W >= 16: equal ranges connect, 10 m against
    20 m does not, and nothing is ground at ground_angle = 1e-9."""
    mask = np.asarray(mask, bool)
    H, W = mask.shape
    el = np.radians(line_gap_deg * (np.arange(H) - (H - 1) / 2.0))
    az = 2.0 * np.pi * np.arange(W) / W
    d = np.stack([np.cos(el)[:, None] * np.cos(az)[None, :], np.cos(el)[:, None] * np.sin(az)[None, :], np.broadcast_to(np.sin(el)[:, None], (H, W))], -1)
    r = np.where(mask, near, 0.0 if far is None else far)
    return np.ascontiguousarray((d * r[..., None]).reshape(-1, 3))


MASK_PARAMS = dict(ground_angle=1e-9)  # nothing on a sphere about the sensor is ground


def random_mask(H, W, seed, density=0.55):
    return np.random.default_rng([H, W, seed]).random((H, W)) < density


def serpentine(H, W):
    """even lines full, odd lines with one linking cell at alternating ends: one component that winds through every tile"""
    m = np.zeros((H, W), bool)
    m[0::2] = True
    for l in range(1, H, 2):
        m[l, W - 2 if (l // 2) % 2 == 0 else 1] = True
    return m


def comb(H, W):
    """vertical teeth joined only along the top line"""
    m = np.zeros((H, W), bool)
    m[:, 0::2] = True
    m[H - 1] = True
    return m


def alternating_lines(H, W):
    return np.broadcast_to((np.arange(H) % 2 == 0)[:, None], (H, W)).copy()


def checkerboard(H, W):
    return (np.arange(H)[:, None] + np.arange(W)[None, :]) % 2 == 0


def floor_scan(H, W, height=1.8):
    """a flat floor under a downward fan (-2 to -30 degrees): all ground, no nodes"""
    el = np.radians(-30.0 + 28.0 * np.arange(H) / max(H - 1, 1))
    az = 2.0 * np.pi * np.arange(W) / W
    r = height / -np.sin(el)
    d = np.stack([np.cos(el)[:, None] * np.cos(az)[None, :], np.cos(el)[:, None] * np.sin(az)[None, :], np.broadcast_to(np.sin(el)[:, None], (H, W))], -1)
    return np.ascontiguousarray((d * r[:, None, None]).reshape(-1, 3))


def real_scan(name, H=32, W=512, dtype=np.float64):
    import outdoor_scenes as S
    origin, yaw = S.sensor_origin(name, 0)
    return np.ascontiguousarray(S.scan_at(name, 0, origin, yaw, H=H, W=W, noise_seed=0).astype(dtype))


def five_scans(H, W):
    """three ray-cast scenes and two masks on a sphere, (5, H W, 3) float64: what the batch tests segment"""
    return np.stack([real_scan("canyon", H, W), mask_scan(random_mask(H, W, 5)), real_scan("field", H, W), mask_scan(serpentine(H, W)),
                     real_scan("lot", H, W)])
