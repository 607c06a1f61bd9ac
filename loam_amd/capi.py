"""ctypes binding of libloamx.so — the C ABI declared in include/loamx.h.

This is host plumbing only: every compute call goes to the HIP kernels through the C ABI. If the
library is missing it raises; there is no Python or CPU fallback.
"""
import collections
import ctypes as C
import os

import numpy as np

from . import build as _build

OK, ERR_SCAN_SIZE, ERR_BAD_PARAM, ERR_HIP, ERR_CAPACITY, ERR_UNSUPPORTED, ERR_NO_DEVICE, ERR_COMM = range(8)
CONVERGED, MAX_ITER, INSUFFICIENT_ASSOCIATIONS = 0, 1, 2
K_CURVATURE, K_SELECT, K_COMPACT, K_GRID, K_ASSOC, K_SWEEP, K_LM, K_MOMENT, K_KNN_PLANE, K_EXTRACT_FUSED, K_INFORMATION, K_CLOUD_ACCUMULATE, K_CLOUD_ACCUMULATE_PLAIN, K_CLOUD_LIST, K_CLOUD_EMIT, K_COUNT = range(16)


class LidarParams(C.Structure):
    """loam::LidarParams (reference: loam/include/loam/common.h:29-41)"""
    _fields_ = [("scan_lines", C.c_uint64), ("points_per_line", C.c_uint64), ("min_range", C.c_double),
                ("max_range", C.c_double)]


class FeatureExtractionParams(C.Structure):
    """loam::FeatureExtractionParams (reference: loam/include/loam/features.h:37-66)"""
    _fields_ = [("neighbor_points", C.c_uint64), ("number_sectors", C.c_uint64),
                ("max_edge_feats_per_sector", C.c_uint64), ("max_planar_feats_per_sector", C.c_uint64),
                ("edge_feat_threshold", C.c_double), ("planar_feat_threshold", C.c_double),
                ("occlusion_thresh", C.c_double), ("parallel_thresh", C.c_double)]

    def __init__(self, *a, **kw):
        if not a and not kw:
            a = (3, 6, 10, 50, 100.0, 1.0, 0.5, 1.0)
        super().__init__(*a, **kw)


class RegistrationParams(C.Structure):
    """loam::RegistrationParams (reference: loam/include/loam/registration.h:40-75)"""
    _fields_ = [("num_edge_neighbors", C.c_uint64), ("max_edge_neighbor_dist", C.c_double),
                ("min_line_fit_points", C.c_uint64), ("min_line_condition_number", C.c_double),
                ("num_plane_neighbors", C.c_uint64), ("max_plane_neighbor_dist", C.c_double),
                ("min_plane_fit_points", C.c_uint64), ("max_avg_point_plane_dist", C.c_double),
                ("max_iterations", C.c_uint64), ("rotation_convergence_thresh", C.c_double),
                ("position_convergence_thresh", C.c_double), ("min_associations", C.c_uint64)]

    def __init__(self, *a, **kw):
        if not a and not kw:
            a = (5, 1.0, 3, 10.0, 5, 2.0, 4, 0.1, 10, 1e-3, 1e-2, 100)
        super().__init__(*a, **kw)


class RegResult(C.Structure):
    _fields_ = [("pose", C.c_double * 7), ("termination", C.c_uint32), ("iterations", C.c_uint32)]


class IterInfo(C.Structure):
    _fields_ = [("target_T_source_init", C.c_double * 7), ("estimate_update", C.c_double * 7),
                ("n_edge_associations", C.c_uint32), ("n_plane_associations", C.c_uint32)]


class RegDetail(C.Structure):
    _fields_ = [("iter_info", C.POINTER(IterInfo)), ("n_iter_info", C.c_uint32),
                ("edge_pairs", C.POINTER(C.c_uint32)), ("pairs_cap_edge", C.c_size_t),
                ("n_edge_pairs", C.POINTER(C.c_uint32)), ("plane_pairs", C.POINTER(C.c_uint32)),
                ("pairs_cap_plane", C.c_size_t), ("n_plane_pairs", C.POINTER(C.c_uint32))]


class KernelStat(C.Structure):
    _fields_ = [("launches", C.c_uint64), ("total_ms", C.c_double), ("algorithmic_bytes", C.c_double)]


RESULT_DTYPE = np.dtype([("pose", np.float64, 7), ("termination", np.uint32), ("iterations", np.uint32)])
# loamx_reg_information as a numpy record (696 bytes): arrays of device records come back as this dtype
INFORMATION_DTYPE = np.dtype([("information", np.float64, (6, 6)), ("eigenvalues", np.float64, 6), ("eigenvectors", np.float64, (6, 6)),
                              ("gradient", np.float64, 6), ("weighted_sq_error", np.float64), ("n_edge", np.uint32),
                              ("n_plane", np.uint32), ("n_huber", np.uint32), ("n_dropped", np.uint32)])


def information_covariance(eigenvalues, eigenvectors, weighted_sq_error, n_rows, rel_threshold=1e-12):
    """sigma^2 * sum v_i v_i^T / lambda_i over lambda_i > rel_threshold * lambda_5, sigma^2 = weighted_sq_error / (n_rows - 6):
    the covariance of the pose in the basis of the information matrix, restricted to the directions the geometry observes."""
    if n_rows <= 6:
        raise ValueError(f"covariance: {n_rows} residual rows do not determine 6 degrees of freedom and a variance")
    lam, vec = np.asarray(eigenvalues, dtype=np.float64), np.asarray(eigenvectors, dtype=np.float64).reshape(6, 6)
    sigma2 = float(weighted_sq_error) / (n_rows - 6)
    cov = np.zeros((6, 6))
    for i in range(6):
        if lam[i] > rel_threshold * lam[5]:
            cov += np.outer(vec[i], vec[i]) / lam[i]
    return sigma2 * cov


class RegInformation(C.Structure):
    """loamx_reg_information (include/loamx.h): the Gauss-Newton information matrix of a pair's residuals at a pose, in the
    left-perturbation basis [omega (rad, target axes), t (m)], with its eigenpairs."""
    _fields_ = [("_information", C.c_double * 36), ("_eigenvalues", C.c_double * 6), ("_eigenvectors", C.c_double * 36),
                ("_gradient", C.c_double * 6), ("weighted_sq_error", C.c_double), ("n_edge", C.c_uint32), ("n_plane", C.c_uint32),
                ("n_huber", C.c_uint32), ("n_dropped", C.c_uint32)]

    @classmethod
    def from_record(cls, rec):
        """from one INFORMATION_DTYPE record (or 696 bytes)"""
        return cls.from_buffer_copy(np.ascontiguousarray(rec).tobytes())

    def _view(self, name, shape):
        return np.ctypeslib.as_array(getattr(self, name)).reshape(shape)

    @property
    def information(self):
        """H = sum J^T J, (6, 6), a view of the record"""
        return self._view("_information", (6, 6))

    @property
    def eigenvalues(self):
        return self._view("_eigenvalues", (6,))

    @property
    def eigenvectors(self):
        """(6, 6): row i is the unit eigenvector of eigenvalues[i]"""
        return self._view("_eigenvectors", (6, 6))

    @property
    def gradient(self):
        return self._view("_gradient", (6,))

    def covariance(self, rel_threshold=1e-12):
        return information_covariance(self.eigenvalues, self.eigenvectors, self.weighted_sq_error, int(self.n_edge) + int(self.n_plane),
                                      rel_threshold)

    def degenerate_directions(self, min_eigenvalue):
        """the eigenvectors (rows) whose eigenvalue lies below min_eigenvalue: the directions the geometry does not constrain"""
        return self.eigenvectors[self.eigenvalues < min_eigenvalue].copy()

class AssocDump(C.Structure):
    """loamx_assoc_dump (include/loamx.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("edge_nn_count", "edge_nn_idx", "edge_valid", "edge_moved", "edge_lines",
                                          "plane_nn_count", "plane_nn_idx", "plane_valid", "plane_moved", "plane_planes", "queue_lengths")]


ORGANIZE_KEEP_FIRST, ORGANIZE_KEEP_NEAREST = 0, 1
NO_POINT = 0xFFFFFFFF  # src_idx of a cell without a winner


class OrganizeParamsStruct(C.Structure):
    """loamx_organize_params (include/loamx.h)"""
    _fields_ = [("azimuth_zero", C.c_double), ("clockwise", C.c_uint32), ("keep", C.c_uint32), ("elevations", C.POINTER(C.c_double)),
                ("fov_bottom", C.c_double), ("fov_top", C.c_double), ("ring_map", C.POINTER(C.c_uint16)), ("n_ring_map", C.c_size_t)]


class OrganizeParams:
    """How an unordered cloud maps onto the scan grid (loamx_organize_params): azimuth of column 0 and sense of rotation, the
    beams' elevations (an array of scan_lines ascending angles in radians, or None: linear from fov_bottom to fov_top), an
    optional ring_map (ring number -> line, 0xFFFF drops the ring) and the winner of a cell (ORGANIZE_KEEP_FIRST / _NEAREST)."""

    def __init__(self, azimuth_zero=0.0, clockwise=False, keep=ORGANIZE_KEEP_FIRST, elevations=None, fov_bottom=None, fov_top=None,
                 ring_map=None):
        d = OrganizeParamsStruct()
        load().loamx_default_organize_params(C.byref(d))
        self.azimuth_zero, self.clockwise, self.keep = float(azimuth_zero), bool(clockwise), int(keep)
        self.elevations = None if elevations is None else np.ascontiguousarray(elevations, dtype=np.float64).reshape(-1)
        self.fov_bottom = d.fov_bottom if fov_bottom is None else float(fov_bottom)
        self.fov_top = d.fov_top if fov_top is None else float(fov_top)
        self.ring_map = None if ring_map is None else np.ascontiguousarray(ring_map, dtype=np.uint16).reshape(-1)

    def struct(self, scan_lines):
        """the C struct (it points into this object's arrays: keep the object alive while the struct is in use)"""
        if self.elevations is not None and self.elevations.size != scan_lines:
            raise ValueError(f"OrganizeParams: {self.elevations.size} elevations for {scan_lines} scan lines")
        if self.keep < 0 or self.keep > 0xFFFFFFFF:
            raise ValueError("OrganizeParams: keep is one of ORGANIZE_KEEP_FIRST, ORGANIZE_KEEP_NEAREST")
        return OrganizeParamsStruct(self.azimuth_zero, 1 if self.clockwise else 0, self.keep,
                                    self.elevations.ctypes.data_as(C.POINTER(C.c_double)) if self.elevations is not None else None,
                                    self.fov_bottom, self.fov_top,
                                    self.ring_map.ctypes.data_as(C.POINTER(C.c_uint16)) if self.ring_map is not None and self.ring_map.size else None,
                                    0 if self.ring_map is None else self.ring_map.size)


class PlaceParamsStruct(C.Structure):
    """loamx_place_params (include/loamx.h)"""
    _fields_ = [("n_rings", C.c_uint32), ("n_sectors", C.c_uint32), ("max_range", C.c_double), ("z_offset", C.c_double),
                ("z_scale", C.c_double)]


class PlaceParams:
    """The shape and scaling of a scan descriptor (loamx_place_params): n_rings x n_sectors cells out to max_range, heights
    counted from z_offset below the sensor in steps of 1 / z_scale. Anything left out takes the C ABI's default."""

    def __init__(self, n_rings=None, n_sectors=None, max_range=None, z_offset=None, z_scale=None):
        d = PlaceParamsStruct()
        load().loamx_default_place_params(C.byref(d))
        self.n_rings = d.n_rings if n_rings is None else int(n_rings)
        self.n_sectors = d.n_sectors if n_sectors is None else int(n_sectors)
        self.max_range = d.max_range if max_range is None else float(max_range)
        self.z_offset = d.z_offset if z_offset is None else float(z_offset)
        self.z_scale = d.z_scale if z_scale is None else float(z_scale)

    def struct(self):
        for name in ("n_rings", "n_sectors"):
            if not 0 <= getattr(self, name) <= 0xFFFFFFFF:
                raise ValueError(f"PlaceParams: {name} does not fit 32 bits")
        return PlaceParamsStruct(self.n_rings, self.n_sectors, self.max_range, self.z_offset, self.z_scale)


# loamx_place_match: one record of a search
PLACE_MATCH_DTYPE = np.dtype([("id", np.uint32), ("shift", np.uint32), ("key_dist", np.uint64), ("distance", np.float64)])
PLACE_NO_ID = 0xFFFFFFFF  # id of a record without an entry (fewer eligible entries than candidates asked for)


class CloudMapParamsStruct(C.Structure):
    """loamx_cloud_map_params (include/loamx.h)"""
    _fields_ = [("leaf", C.c_double), ("min_range", C.c_double), ("max_range", C.c_double)]


class CloudMapParams:
    """The rule of a cloud map (loamx_cloud_map_params): voxel edge, and the range band outside which a point is dropped.
    Anything left out takes the C ABI's default."""

    def __init__(self, leaf=None, min_range=None, max_range=None):
        d = CloudMapParamsStruct()
        load().loamx_default_cloud_map_params(C.byref(d))
        self.leaf = d.leaf if leaf is None else float(leaf)
        self.min_range = d.min_range if min_range is None else float(min_range)
        self.max_range = d.max_range if max_range is None else float(max_range)

    def struct(self):
        return CloudMapParamsStruct(float(self.leaf), float(self.min_range), float(self.max_range))


class LocalizeParamsStruct(C.Structure):
    """loamx_localize_params (include/loamx.h, "surfel localisation"): 64 bytes"""
    _fields_ = [("neighborhood", C.c_uint32), ("min_points", C.c_uint32), ("planarity", C.c_double), ("max_distance", C.c_double),
                ("huber_delta", C.c_double), ("max_iterations", C.c_uint32), ("min_rows", C.c_uint32),
                ("rotation_convergence_thresh", C.c_double), ("position_convergence_thresh", C.c_double), ("min_eigenvalue_per_row", C.c_double)]


class LocalizeParams:
    """The parameters of a localisation call (loamx_localize_params). Anything left out takes the C ABI's default."""
    _NAMES = tuple(f[0] for f in LocalizeParamsStruct._fields_)
    _INTS = ("neighborhood", "min_points", "max_iterations", "min_rows")

    def __init__(self, **kw):
        d = LocalizeParamsStruct()
        load().loamx_default_localize_params(C.byref(d))
        unknown = set(kw) - set(self._NAMES)
        if unknown:
            raise ValueError(f"LocalizeParams: unknown parameter {sorted(unknown)}")
        for n in self._NAMES:
            setattr(self, n, getattr(d, n) if kw.get(n) is None else kw[n])

    def struct(self):
        for n in self._INTS:
            if not 0 <= int(getattr(self, n)) <= 0xFFFFFFFF:
                raise ValueError(f"LocalizeParams: {n} does not fit 32 bits")
        return LocalizeParamsStruct(*[int(getattr(self, n)) if n in self._INTS else float(getattr(self, n)) for n in self._NAMES])


# loamx_localize_result (128 bytes) and its termination codes
LOCALIZE_RESULT_DTYPE = np.dtype([("pose", np.float64, 7), ("initial_cost", np.float64), ("final_cost", np.float64), ("last_rotation", np.float64),
                                  ("last_translation", np.float64), ("iterations", np.uint32), ("termination", np.uint32), ("n_rows", np.uint32),
                                  ("n_huber", np.uint32), ("n_no_surfel", np.uint32), ("n_gated", np.uint32), ("n_unused", np.uint32),
                                  ("used_mask", np.uint32), ("n_rows_initial", np.uint32), ("reserved", np.uint32)])
assert LOCALIZE_RESULT_DTYPE.itemsize == 128
LOCALIZE_CONVERGED, LOCALIZE_MAX_ITERATIONS, LOCALIZE_TOO_FEW_ROWS, LOCALIZE_NOT_FINITE = 0, 1, 2, 3


# loamx_cloud_map_stats
CLOUD_MAP_STATS_DTYPE = np.dtype([(n, np.uint64) for n in ("voxels", "points_offered", "points_used", "invalid", "range", "outside", "overflow")])


class SurfelMapParamsStruct(C.Structure):
    """loamx_surfel_map_params (include/loamx.h)"""
    _fields_ = [("leaf", C.c_double), ("min_range", C.c_double), ("max_range", C.c_double)]


class SurfelMapParams:
    """The rule of a surfel map (loamx_surfel_map_params): voxel edge, and the range band outside which a point is dropped.
    Anything left out takes the C ABI's default."""

    def __init__(self, leaf=None, min_range=None, max_range=None):
        d = SurfelMapParamsStruct()
        load().loamx_default_surfel_map_params(C.byref(d))
        self.leaf = d.leaf if leaf is None else float(leaf)
        self.min_range = d.min_range if min_range is None else float(min_range)
        self.max_range = d.max_range if max_range is None else float(max_range)

    def struct(self):
        return SurfelMapParamsStruct(float(self.leaf), float(self.min_range), float(self.max_range))


# loamx_surfel (128 bytes) and loamx_surfel_map_stats
SURFEL_DTYPE = np.dtype([("mean", np.float64, 3), ("cov", np.float64, 6), ("eval", np.float64, 3), ("normal", np.float64, 3),
                         ("count", np.uint32), ("first", np.uint32)])
SURFEL_MAP_STATS_DTYPE = np.dtype([(n, np.uint64) for n in ("voxels", "points_offered", "points_used", "invalid", "range", "outside", "overflow")])


class OccupancyParamsStruct(C.Structure):
    """loamx_occupancy_params (include/loamx.h)"""
    _fields_ = [("leaf", C.c_double), ("min_range", C.c_double), ("max_range", C.c_double), ("end_margin", C.c_double),
                ("clip_long", C.c_uint32), ("min_hits", C.c_uint32), ("occ_ratio", C.c_double), ("min_passes", C.c_uint32)]


class OccupancyParams:
    """The rule of an occupancy map (loamx_occupancy_params): voxel edge, range band, how far in front of a return a walk stops,
    whether rays beyond max_range are walked up to it, and the three thresholds of a voxel's state. Anything left out takes
    the C ABI's default."""
    NAMES = ("leaf", "min_range", "max_range", "end_margin", "clip_long", "min_hits", "occ_ratio", "min_passes")

    def __init__(self, leaf=None, min_range=None, max_range=None, end_margin=None, clip_long=None, min_hits=None, occ_ratio=None, min_passes=None):
        d = OccupancyParamsStruct()
        load().loamx_default_occupancy_params(C.byref(d))
        given = dict(leaf=leaf, min_range=min_range, max_range=max_range, end_margin=end_margin, clip_long=clip_long, min_hits=min_hits,
                     occ_ratio=occ_ratio, min_passes=min_passes)
        for name in self.NAMES:
            setattr(self, name, getattr(d, name) if given[name] is None else given[name])

    def struct(self):
        for name in ("clip_long", "min_hits", "min_passes"):
            if not 0 <= int(getattr(self, name)) <= 0xFFFFFFFF:
                raise ValueError(f"OccupancyParams: {name} does not fit 32 bits")
        return OccupancyParamsStruct(float(self.leaf), float(self.min_range), float(self.max_range), float(self.end_margin), int(self.clip_long),
                                     int(self.min_hits), float(self.occ_ratio), int(self.min_passes))


# loamx_occupancy_stats
OCCUPANCY_STATS_DTYPE = np.dtype([(n, np.uint64) for n in ("rays_offered", "rays_hit", "invalid", "range_short", "range_long", "outside", "visits",
                                                          "voxels", "overflow")])
OCC_UNKNOWN, OCC_FREE, OCC_OCCUPIED = 0, 1, 2  # LOAMX_OCC_*: the state of a voxel
DIST_FAR = 0xFFFF  # LOAMX_DIST_FAR: the squared distance of a voxel with no obstacle within max_dist_voxels


class DistanceParamsStruct(C.Structure):
    """loamx_distance_params (include/loamx.h)"""
    _fields_ = [("max_dist_voxels", C.c_uint32), ("unknown_is_obstacle", C.c_uint32)]


class DistanceParams:
    """The rule of an occupancy distance field (loamx_distance_params): the cap R in voxels (1 .. 255) and whether UNKNOWN voxels
    are obstacles. Anything left out takes the C ABI's default."""
    NAMES = ("max_dist_voxels", "unknown_is_obstacle")

    def __init__(self, max_dist_voxels=None, unknown_is_obstacle=None):
        d = DistanceParamsStruct()
        load().loamx_default_distance_params(C.byref(d))
        self.max_dist_voxels = d.max_dist_voxels if max_dist_voxels is None else max_dist_voxels
        self.unknown_is_obstacle = d.unknown_is_obstacle if unknown_is_obstacle is None else unknown_is_obstacle

    def struct(self):
        if not 0 <= int(self.max_dist_voxels) <= 0xFFFFFFFF:
            raise ValueError("DistanceParams: max_dist_voxels does not fit 32 bits")
        return DistanceParamsStruct(int(self.max_dist_voxels), 1 if self.unknown_is_obstacle else 0)


class RaycastParamsStruct(C.Structure):
    """loamx_raycast_params (include/loamx.h)"""
    _fields_ = [("skip_start", C.c_uint32), ("unknown_stops", C.c_uint32), ("max_steps", C.c_uint32), ("hit_at", C.c_uint32)]


# LOAMX_RAY_*: the status of a ray, and where on the hit voxel a rendered return lies
RAY_CLEAR, RAY_HIT, RAY_UNKNOWN, RAY_TRUNCATED, RAY_OUTSIDE, RAY_INVALID = range(6)
RAY_AT_ENTER, RAY_AT_MIDDLE = 0, 1
# loamx_ray_record (40 bytes) and loamx_raycast_census
RAY_RECORD_DTYPE = np.dtype([("status", np.uint32), ("visits", np.uint32), ("voxel", np.int32, 3), ("n_unknown", np.uint32),
                             ("t_enter", np.float64), ("t_exit", np.float64)])
RAYCAST_CENSUS_DTYPE = np.dtype([(n, np.uint64) for n in ("rays", "visits", "probes", "hit", "unknown", "clear", "truncated", "outside", "invalid")])


class RaycastParams:
    """The rule of a ray cast through an occupancy map (loamx_raycast_params): visits at the start that are walked but not tested,
    whether an UNKNOWN voxel stops a ray, the step cap, and where on the hit voxel a rendered return lies (RAY_AT_ENTER /
    RAY_AT_MIDDLE). Anything left out takes the C ABI's default."""
    NAMES = ("skip_start", "unknown_stops", "max_steps", "hit_at")

    def __init__(self, skip_start=None, unknown_stops=None, max_steps=None, hit_at=None):
        d = RaycastParamsStruct()
        load().loamx_default_raycast_params(C.byref(d))
        given = dict(skip_start=skip_start, unknown_stops=unknown_stops, max_steps=max_steps, hit_at=hit_at)
        for name in self.NAMES:
            setattr(self, name, getattr(d, name) if given[name] is None else given[name])

    def struct(self):
        for name in self.NAMES:
            if not 0 <= int(getattr(self, name)) <= 0xFFFFFFFF:
                raise ValueError(f"RaycastParams: {name} does not fit 32 bits")
        return RaycastParamsStruct(int(self.skip_start), 1 if self.unknown_stops else 0, int(self.max_steps), int(self.hit_at))


def beam_directions(scan_lines, points_per_line, organize_params=None):
    """(scan_lines * points_per_line, 3) float64: the unit directions of the CENTRES of a scan layout's cells, in cell order (line
    major), for OccupancyMap.render_scans. Column c is centred on azimuth_zero + sgn 2 pi c / W (its boundaries lie half a column to
    either side: loamx_organize_params), line l on its elevation: the given elevations, or linear from fov_bottom to fov_top."""
    o = organize_params or OrganizeParams()
    H, W = int(scan_lines), int(points_per_line)
    if o.elevations is not None:
        if o.elevations.size != H:
            raise ValueError(f"beam_directions: {o.elevations.size} elevations for {H} scan lines")
        el = o.elevations.astype(np.float64)
    else:
        el = np.array([o.fov_bottom + (o.fov_top - o.fov_bottom) * l / (H - 1) if H > 1 else 0.5 * (o.fov_bottom + o.fov_top) for l in range(H)])
    az = o.azimuth_zero + (-1.0 if o.clockwise else 1.0) * (2.0 * np.pi * np.arange(W) / W)
    d = np.stack([np.cos(el)[:, None] * np.cos(az)[None, :], np.cos(el)[:, None] * np.sin(az)[None, :],
                  np.sin(el)[:, None] * np.ones(W)[None, :]], axis=-1).reshape(H * W, 3)
    return np.ascontiguousarray(d / np.linalg.norm(d, axis=1)[:, None])


class SegmentParamsStruct(C.Structure):
    """loamx_segment_params (include/loamx.h)"""
    _fields_ = [("ground_lines", C.c_uint64), ("ground_angle", C.c_double), ("segment_angle", C.c_double),
                ("min_cluster_points", C.c_uint64), ("min_tall_cluster_points", C.c_uint64), ("min_tall_cluster_lines", C.c_uint64),
                ("drop_outliers", C.c_uint32), ("drop_ground", C.c_uint32)]


class SegmentParams:
    """The rule of the scan segmentation (loamx_segment_params): the lines that can be ground and the ground angle, the
    segmentation angle, the accept rule of a component and what the filtered scan drops. Anything left out takes the C ABI's
    default."""
    FIELDS = tuple(f[0] for f in SegmentParamsStruct._fields_)

    def __init__(self, **kw):
        d = SegmentParamsStruct()
        load().loamx_default_segment_params(C.byref(d))
        for name in self.FIELDS:
            setattr(self, name, getattr(d, name))
        for name, v in kw.items():
            if name not in self.FIELDS:
                raise TypeError(f"SegmentParams: no field {name}")
            setattr(self, name, v)

    def struct(self):
        for name in ("ground_lines", "min_cluster_points", "min_tall_cluster_points", "min_tall_cluster_lines"):
            if int(getattr(self, name)) < 0:
                raise ValueError(f"SegmentParams: {name} must be >= 0")
        return SegmentParamsStruct(int(self.ground_lines), float(self.ground_angle), float(self.segment_angle), int(self.min_cluster_points),
                                   int(self.min_tall_cluster_points), int(self.min_tall_cluster_lines), 1 if self.drop_outliers else 0,
                                   1 if self.drop_ground else 0)


# classes of a cell, the label of a cell without a component, loamx_segment_cluster, the names of the stats words
SEGMENT_INVALID, SEGMENT_GROUND, SEGMENT_CLUSTER, SEGMENT_OUTLIER = 0, 1, 2, 3
SEGMENT_NO_LABEL = 0xFFFFFFFF
SEGMENT_CLUSTER_DTYPE = np.dtype([("root", np.uint32), ("size", np.uint32), ("line_min", np.uint32), ("line_max", np.uint32)])
SEGMENT_STATS = ("invalid", "ground", "cluster_cells", "outlier_cells", "accepted", "rejected", "largest", "records")
SegmentCensus = collections.namedtuple("SegmentCensus", "tile_lines tile_cols tiles_per_scan merged_edges tiles")


def segment_constants(params=None):
    """(tg2, c2) = (tan(ground_angle)^2, cos(segment_angle)^2) exactly as the launcher computes them (loamx_segment_constants)"""
    st = (params or SegmentParams()).struct()
    out = (C.c_double * 2)()
    rc = load().loamx_segment_constants(C.byref(st), out)
    if rc != OK:
        raise LoamxError(rc, "loamx_segment_constants: " + load().loamx_status_string(rc).decode())
    return float(out[0]), float(out[1])


class VisibilityParamsStruct(C.Structure):
    """loamx_visibility_params (include/loamx.h)"""
    _fields_ = [("min_range", C.c_double), ("max_range", C.c_double), ("margin", C.c_double), ("margin_rel", C.c_double),
                ("window_lines", C.c_uint32), ("window_cols", C.c_uint32), ("min_through", C.c_uint32), ("through_ratio", C.c_double)]


class VisibilityParams:
    """The rule of the map cleaning (loamx_visibility_params): the range band in which a scan can vote on a point, the margin around
    the point's range, the window of cells looked at, and the decision over the votes. Anything left out takes the C ABI's default."""
    FIELDS = tuple(f[0] for f in VisibilityParamsStruct._fields_)
    INTEGERS = ("window_lines", "window_cols", "min_through")

    def __init__(self, **kw):
        d = VisibilityParamsStruct()
        load().loamx_default_visibility_params(C.byref(d))
        for name in self.FIELDS:
            setattr(self, name, getattr(d, name))
        for name, v in kw.items():
            if name not in self.FIELDS:
                raise TypeError(f"VisibilityParams: no field {name}")
            setattr(self, name, v)

    def struct(self):
        for name in self.INTEGERS:
            if not 0 <= int(getattr(self, name)) <= 0xFFFFFFFF:
                raise ValueError(f"VisibilityParams: {name} does not fit 32 bits")
        return VisibilityParamsStruct(*(int(getattr(self, n)) if n in self.INTEGERS else float(getattr(self, n)) for n in self.FIELDS))


# loamx_visibility_tally: the votes of one map point; loamx_visibility_census
VISIBILITY_VOTES_DTYPE = np.dtype([("through", np.uint32), ("agree", np.uint32), ("occluded", np.uint32), ("empty", np.uint32)])
VISIBILITY_SCAN_CHUNK = 32  # scans per workgroup row of the votes kernel


class VisibilityCensusStruct(C.Structure):
    _fields_ = [("form", C.c_uint32), ("scan_chunks", C.c_uint32), ("in_range_pairs", C.c_uint64), ("projected_pairs", C.c_uint64)]


VisibilityCensus = collections.namedtuple("VisibilityCensus", "form scan_chunks in_range_pairs projected_pairs")


class PgoParamsStruct(C.Structure):
    """loamx_pgo_params (include/loamx.h)"""
    _fields_ = [("max_iterations", C.c_uint32), ("max_pcg_iterations", C.c_uint32), ("pcg_tolerance", C.c_double),
                ("initial_lambda", C.c_double), ("cost_tolerance", C.c_double), ("step_tolerance", C.c_double),
                ("huber_delta", C.c_double)]


class PgoParams:
    """The parameters of a pose-graph solve (loamx_pgo_params). Anything left out takes the C ABI's default."""
    FIELDS = tuple(f[0] for f in PgoParamsStruct._fields_)

    def __init__(self, **kw):
        d = PgoParamsStruct()
        load().loamx_pgo_default_params(C.byref(d))
        for name in self.FIELDS:
            setattr(self, name, getattr(d, name))
        for name, v in kw.items():
            if name not in self.FIELDS:
                raise TypeError(f"PgoParams has no field {name}")
            setattr(self, name, v)

    def struct(self):
        for name in self.FIELDS[:2]:
            if not 0 <= int(getattr(self, name)) <= 0xFFFFFFFF:
                raise ValueError(f"PgoParams: {name} does not fit 32 bits")
        return PgoParamsStruct(int(self.max_iterations), int(self.max_pcg_iterations), *(float(getattr(self, n)) for n in self.FIELDS[2:]))


# loamx_pgo_edge, loamx_pgo_summary, loamx_pgo_linearization
PGO_EDGE_DTYPE = np.dtype([("a", np.uint32), ("b", np.uint32), ("a_T_b", np.float64, 7), ("information", np.float64, (6, 6))])
PGO_SUMMARY_DTYPE = np.dtype([("initial_cost", np.float64), ("final_cost", np.float64), ("lambda", np.float64), ("max_update", np.float64),
                              ("iterations", np.uint32), ("accepted", np.uint32), ("pcg_iterations", np.uint32),
                              ("termination", np.uint32), ("n_bad_edges", np.uint32), ("reserved", np.uint32)])
PGO_LINEARIZATION_DTYPE = np.dtype([("e", np.float64, 6), ("chi2", np.float64), ("weight", np.float64), ("A", np.float64, (6, 6)),
                                    ("B", np.float64, (6, 6))])
PGO_TERMINATIONS = ("COST_CONVERGED", "STEP_CONVERGED", "MAX_ITERATIONS", "LAMBDA_OVERFLOW", "NOTHING_TO_DO", "BAD_INPUT")
(PGO_COST_CONVERGED, PGO_STEP_CONVERGED, PGO_MAX_ITERATIONS, PGO_LAMBDA_OVERFLOW, PGO_NOTHING_TO_DO, PGO_BAD_INPUT) = range(6)


EXPORTS = [
    "loamx_default_fe_params", "loamx_default_reg_params", "loamx_status_string", "loamx_last_error",
    "loamx_ctx_create", "loamx_ctx_destroy", "loamx_ctx_set_stream", "loamx_ctx_synchronize",
    "loamx_compute_curvature", "loamx_compute_valid_points", "loamx_extract_features", "loamx_register_features",
    "loamx_target_index_create", "loamx_target_index_destroy", "loamx_register_features_indexed",
    "loamx_edge_capacity", "loamx_planar_capacity", "loamx_extract_features_batch_dev",
    "loamx_register_features_batch_dev", "loamx_register_scan_pairs_dev", "loamx_register_scan_pairs",
    "loamx_register_scan_pairs_f32", "loamx_ctx_enable_kernel_timing",
    "loamx_ctx_reset_kernel_stats", "loamx_ctx_get_kernel_stats", "loamx_kernel_name", "loamx_synth_pair_pose",
    "loamx_synth_scan_host", "loamx_synth_scan_pairs_dev", "loamx_dev_alloc", "loamx_dev_free",
    "loamx_copy_to_device", "loamx_copy_to_host",
    "loamx_compute_curvature_f32", "loamx_compute_valid_points_f32", "loamx_extract_features_f32",
    "loamx_extract_features_batch_dev_f32", "loamx_register_scan_pairs_dev_f32",
    "loamx_target_index_insert", "loamx_target_index_size", "loamx_target_index_census",
    "loamx_shard_range", "loamx_comm_get_unique_id", "loamx_comm_create", "loamx_comm_wrap", "loamx_comm_destroy",
    "loamx_comm_info", "loamx_gather_results_dev", "loamx_comm_barrier", "loamx_comm_stats", "loamx_ctx_extract_counters",
    "loamx_ctx_set_option", "loamx_ctx_get_option", "loamx_ctx_last_extract_route", "loamx_ctx_last_solve_census",
    "loamx_ctx_last_assoc_census",
    "loamx_ctx_last_assoc_coop_forms",
    "loamx_fit_lines", "loamx_fit_planes", "loamx_knn_search", "loamx_associate", "loamx_target_index_stats",
    "loamx_register_scan_sequence_dev", "loamx_register_scan_sequence_dev_f32", "loamx_register_scan_sequence",
    "loamx_register_scan_sequence_f32", "loamx_compose_trajectory_dev", "loamx_deskew_scans_dev", "loamx_deskew_scans_dev_f32",
    "loamx_deskew_launch_geometry",
    "loamx_target_index_points", "loamx_voxel_filter_dev", "loamx_target_index_insert_filtered", "loamx_target_index_crop",
    "loamx_registration_information", "loamx_registration_information_indexed", "loamx_registration_information_batch_dev",
    "loamx_register_scan_pairs_info_dev", "loamx_register_scan_pairs_info_dev_f32", "loamx_register_scan_sequence_info_dev",
    "loamx_register_scan_sequence_info_dev_f32",
    "loamx_default_organize_params", "loamx_scan_layout_create", "loamx_scan_layout_destroy", "loamx_scan_layout_tables",
    "loamx_organize_clouds_dev", "loamx_organize_clouds_dev_f32", "loamx_organize_cloud", "loamx_organize_cloud_f32",
    "loamx_default_place_params", "loamx_place_db_create", "loamx_place_db_destroy", "loamx_place_db_sector_dirs", "loamx_place_db_size",
    "loamx_place_descriptors_dev", "loamx_place_descriptors_dev_f32", "loamx_place_db_add_dev", "loamx_place_db_read",
    "loamx_place_search_dev", "loamx_place_descriptor", "loamx_place_descriptor_f32", "loamx_place_search",
    "loamx_pgo_default_params", "loamx_pose_graph_optimize_dev", "loamx_pose_graph_optimize", "loamx_pose_graph_linearize",
    "loamx_pose_graph_edges_from_results_dev",
    "loamx_default_cloud_map_params", "loamx_cloud_map_create", "loamx_cloud_map_destroy", "loamx_cloud_map_clear",
    "loamx_cloud_map_add_clouds_dev", "loamx_cloud_map_add_clouds_dev_f32", "loamx_cloud_map_emit_dev", "loamx_cloud_map_stats_read",
    "loamx_cloud_map_add_cloud", "loamx_cloud_map_add_cloud_f32", "loamx_cloud_map_emit", "loamx_cloud_map_claims_read",
    "loamx_default_segment_params", "loamx_segment_constants", "loamx_segment_scans_dev", "loamx_segment_scans_dev_f32",
    "loamx_segment_scan", "loamx_segment_scan_f32", "loamx_ctx_last_segment_census",
    "loamx_default_visibility_params", "loamx_visibility_votes_dev", "loamx_visibility_votes_dev_f32", "loamx_visibility_filter_dev",
    "loamx_visibility_votes", "loamx_visibility_votes_f32", "loamx_ctx_last_visibility_census",
    "loamx_default_occupancy_params", "loamx_occupancy_create", "loamx_occupancy_destroy", "loamx_occupancy_clear",
    "loamx_occupancy_add_clouds_dev", "loamx_occupancy_add_clouds_dev_f32", "loamx_occupancy_query_dev", "loamx_occupancy_box_dev",
    "loamx_occupancy_slice_dev", "loamx_occupancy_stats_read", "loamx_occupancy_claims_read", "loamx_occupancy_add_cloud",
    "loamx_occupancy_add_cloud_f32", "loamx_occupancy_query", "loamx_occupancy_box", "loamx_occupancy_slice",
    "loamx_default_surfel_map_params", "loamx_surfel_map_create", "loamx_surfel_map_destroy", "loamx_surfel_map_clear",
    "loamx_surfel_map_add_clouds", "loamx_surfel_map_add_clouds_f32", "loamx_surfel_map_emit", "loamx_surfel_map_query",
    "loamx_surfel_map_stats_read", "loamx_surfel_map_claims_read", "loamx_surfel_map_add_cloud_host", "loamx_surfel_map_add_cloud_host_f32",
    "loamx_surfel_map_emit_host",
    "loamx_default_localize_params", "loamx_surfel_localizer_create", "loamx_surfel_localizer_destroy", "loamx_surfel_localizer_run",
    "loamx_surfel_localizer_run_f32", "loamx_surfel_localizer_run_host", "loamx_surfel_localizer_run_host_f32",
    "loamx_cloud_map_crop", "loamx_surfel_map_crop", "loamx_occupancy_crop",
    "loamx_default_distance_params", "loamx_occupancy_distance_box", "loamx_occupancy_distance_slice",
    "loamx_occupancy_distance_box_host", "loamx_occupancy_distance_slice_host",
    "loamx_default_raycast_params", "loamx_occupancy_cast_rays", "loamx_occupancy_render_scans", "loamx_occupancy_cast_rays_host",
    "loamx_occupancy_render_scans_host", "loamx_ctx_last_raycast_census",
]

# bits of loamx_ctx_last_extract_route (include/loamx.h: LOAMX_ROUTE_*), in bit order
ROUTE_BITS = ("SPLIT_CURV", "CURV2", "CURV_V1", "CURV_GENERIC", "ROWS", "ROWS_CH11", "ROWS_PASS2", "ROWS_LIST16", "MIS", "MIS_4LINES",
              "MIS_TWO", "MIS_CONST_W", "ARGMAX4", "ARGMAX1", "FUSED_COMPACT", "COMPACT", "FUSED_EXTRACT", "FUSED_ROWS", "BOXES")


class ExtractRoute:
    """The route word of the last extraction: `"ROWS" in r`, r.names (the set bits), r.rows_R / r.rows_ch (geometry of the
    row kernels: neighbor_points - 1 and points per lane; 0 when they did not run)."""

    def __init__(self, bits):
        self.bits = int(bits)
        self.names = frozenset(n for i, n in enumerate(ROUTE_BITS) if self.bits >> i & 1)
        self.rows_R = self.bits >> 20 & 7
        self.rows_ch = self.bits >> 24 & 63

    def __contains__(self, name):
        if name not in ROUTE_BITS:
            raise KeyError(name)
        return name in self.names

    def __repr__(self):
        return "ExtractRoute(%s%s)" % ("|".join(n for n in ROUTE_BITS if n in self.names),
                                       ", R=%d ch=%d" % (self.rows_R, self.rows_ch) if "ROWS" in self.names else "")


class SolveCensusStruct(C.Structure):
    """loamx_solve_census (include/loamx.h)"""
    _fields_ = [("iterations", C.c_uint32), ("termination", C.c_uint32), ("use_moments", C.c_uint32), ("mom_ref_on", C.c_uint32),
                ("mom_ref", C.c_double * 7), ("tiles", C.c_uint32), ("live_tiles", C.c_uint32),
                ("edge_stride", C.c_uint64), ("planar_stride", C.c_uint64), ("n_se", C.c_uint32), ("n_sp", C.c_uint32),
                ("walk", C.c_uint32), ("listed_total", C.c_uint32), ("s0max", C.c_double), ("v2max", C.c_double),
                ("sweep_chunk", C.c_uint32), ("edge_cache", C.c_uint32), ("list_cache", C.c_uint32), ("flat_cache", C.c_uint32),
                ("tile_counts", C.POINTER(C.c_uint32)), ("tile_counts_cap", C.c_size_t)]


WALK_NONE, WALK_FLAT, WALK_TILED_BY_COUNT, WALK_TILED_BY_TILES = 0, 1, 2, 3
WALK_NAMES = ("none", "flat", "tiled-by-count", "tiled-by-tiles")
SolveCensus = collections.namedtuple(
    "SolveCensus", "iterations termination use_moments mom_ref_on mom_ref tiles live_tiles edge_stride planar_stride n_se n_sp walk "
                   "listed_total s0max v2max sweep_chunk edge_cache list_cache flat_cache tile_counts")


class AssocCensusStruct(C.Structure):
    """loamx_assoc_census (include/loamx.h)"""
    _fields_ = ([("n_src", C.c_uint32), ("n_tgt", C.c_uint32), ("stride", C.c_uint64)] +
                [(n, C.c_uint32) for n in ("km", "search", "mixed_launch", "one_stage", "leftover_kernel", "rest_blocks", "coop_blocks",
                                           "rest_spread", "left_spread", "lean_set")] +
                [("origin", C.c_double * 3), ("h", C.c_double), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32)] +
                [(n, C.c_uint32) for n in ("n_points", "verified", "unverified", "queued_words", "queued", "queued_plain", "queued_wide",
                                           "queued_tied", "rest_searched", "listed", "leftover_finished", "exact", "late")] +
                [("entry_query", C.POINTER(C.c_uint32)), ("entry_reason", C.POINTER(C.c_uint32)),
                 ("count_after_rest", C.POINTER(C.c_int32)), ("count_before_fit", C.POINTER(C.c_int32)), ("entries_cap", C.c_size_t),
                 ("late_query", C.POINTER(C.c_uint32)), ("late_cap", C.c_size_t)])


ASSOC_SEARCH_NONE, ASSOC_SEARCH_BRUTE, ASSOC_SEARCH_GRID = 0, 1, 2
ASSOC_LEFTOVER_NONE, ASSOC_LEFTOVER_LEFT, ASSOC_LEFTOVER_COOP = 0, 1, 2
ASSOC_REASON_WIDE, ASSOC_REASON_TIED = 0x80000000, 0x40000000
ASSOC_CENSUS_SCALARS = ("n_src n_tgt stride km search mixed_launch one_stage leftover_kernel rest_blocks coop_blocks rest_spread left_spread "
                        "lean_set h nx ny nz n_points verified unverified queued_words queued queued_plain queued_wide queued_tied "
                        "rest_searched listed leftover_finished exact late").split()
AssocCensus = collections.namedtuple("AssocCensus", ASSOC_CENSUS_SCALARS + ["origin", "entry_query", "entry_reason", "count_after_rest",
                                                                            "count_before_fit", "late_query"])


class IndexCensusStruct(C.Structure):
    """loamx_index_census (include/loamx.h)"""
    _fields_ = [("n", C.c_uint64), ("capacity", C.c_uint64), ("origin", C.c_double * 3), ("h", C.c_double), ("inv_h", C.c_double),
                ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("n_points", C.c_uint32),
                ("build", C.c_uint32), ("table_valid", C.c_uint32), ("table_entries", C.c_uint64),
                ("lds_passes", C.c_uint32), ("scan_tiles", C.c_uint32), ("last_op", C.c_uint32), ("reserved", C.c_uint32),
                ("full_builds", C.c_uint64), ("merges", C.c_uint64),
                ("cell_start", C.POINTER(C.c_uint32)), ("cell_start_cap", C.c_size_t),
                ("xyz", C.POINTER(C.c_double)), ("orig", C.POINTER(C.c_uint32)), ("points_cap", C.c_size_t),
                ("rel", C.POINTER(C.c_float)), ("rel_cap", C.c_size_t)]


INDEX_BUILD_NONE, INDEX_BUILD_PACKED, INDEX_BUILD_SINGLE, INDEX_BUILD_BIG = 0, 1, 2, 3
INDEX_BUILD_NAMES = ("none", "packed", "single", "big")
INDEX_OP_NONE, INDEX_OP_FULL_BUILD, INDEX_OP_MERGE = 0, 1, 2
IndexCensus = collections.namedtuple(
    "IndexCensus", "n capacity origin h inv_h dims n_points build table_valid table_entries lds_passes scan_tiles last_op full_builds "
                   "merges cell_start xyz orig rel")


_lib = None


def load(build_if_missing=True):
    """Loads libloamx.so (building it with hipcc if needed). Raises if it cannot be had."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.LIB_PATH
    if build_if_missing and _build.needs_build():
        _build.build()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `python -m loam_amd.build` (no CPU fallback exists)")
    lib = C.CDLL(path)
    dp, u32p, vp = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_void_p
    lib.loamx_status_string.restype = C.c_char_p
    lib.loamx_last_error.restype = C.c_char_p
    lib.loamx_last_error.argtypes = [vp]
    lib.loamx_kernel_name.restype = C.c_char_p
    lib.loamx_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.loamx_ctx_destroy.argtypes = [vp]
    lib.loamx_ctx_destroy.restype = None
    lib.loamx_ctx_set_stream.argtypes = [vp, vp]
    lib.loamx_ctx_synchronize.argtypes = [vp]
    lib.loamx_compute_curvature.argtypes = [vp, dp, C.c_size_t, C.POINTER(LidarParams),
                                            C.POINTER(FeatureExtractionParams), dp]
    lib.loamx_compute_valid_points.argtypes = [vp, dp, C.c_size_t, C.POINTER(LidarParams),
                                               C.POINTER(FeatureExtractionParams), C.POINTER(C.c_uint8)]
    lib.loamx_extract_features.argtypes = [vp, dp, C.c_size_t, C.POINTER(LidarParams),
                                           C.POINTER(FeatureExtractionParams), u32p, C.c_size_t,
                                           C.POINTER(C.c_size_t), u32p, C.c_size_t, C.POINTER(C.c_size_t)]
    fp = C.POINTER(C.c_float)
    lib.loamx_compute_curvature_f32.argtypes = [vp, fp, C.c_size_t, C.POINTER(LidarParams),
                                                C.POINTER(FeatureExtractionParams), dp]
    lib.loamx_compute_valid_points_f32.argtypes = [vp, fp, C.c_size_t, C.POINTER(LidarParams),
                                                   C.POINTER(FeatureExtractionParams), C.POINTER(C.c_uint8)]
    lib.loamx_extract_features_f32.argtypes = [vp, fp, C.c_size_t, C.POINTER(LidarParams),
                                               C.POINTER(FeatureExtractionParams), u32p, C.c_size_t,
                                               C.POINTER(C.c_size_t), u32p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.loamx_register_features.argtypes = [vp, dp, C.c_size_t, dp, C.c_size_t, dp, C.c_size_t, dp, C.c_size_t, dp,
                                            C.POINTER(RegistrationParams), C.POINTER(RegResult),
                                            C.POINTER(RegDetail)]
    lib.loamx_target_index_create.argtypes = [vp, dp, C.c_size_t, dp, C.c_size_t, C.POINTER(RegistrationParams), C.POINTER(vp)]
    lib.loamx_target_index_insert.argtypes = [vp, vp, dp, C.c_size_t, dp, C.c_size_t]
    lib.loamx_target_index_size.argtypes = [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    lib.loamx_target_index_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.loamx_target_index_points.argtypes = [vp, vp, C.c_int, C.c_size_t, C.c_size_t, dp]
    lib.loamx_target_index_census.argtypes = [vp, vp, C.c_int, C.POINTER(IndexCensusStruct)]
    lib.loamx_voxel_filter_dev.argtypes = [vp, vp, C.c_size_t, dp, C.c_double, vp, vp, vp]
    lib.loamx_target_index_insert_filtered.argtypes = [vp, vp, dp, C.c_size_t, dp, C.c_size_t, dp, C.c_double, C.c_double,
                                                       C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    lib.loamx_target_index_crop.argtypes = [vp, vp, dp, dp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    lib.loamx_target_index_destroy.argtypes = [vp, vp]
    lib.loamx_target_index_destroy.restype = None
    lib.loamx_register_features_indexed.argtypes = [vp, vp, dp, C.c_size_t, dp, C.c_size_t, dp, C.POINTER(RegistrationParams),
                                                    C.POINTER(RegResult), C.POINTER(RegDetail)]
    lib.loamx_edge_capacity.restype = C.c_size_t
    lib.loamx_edge_capacity.argtypes = [C.POINTER(LidarParams), C.POINTER(FeatureExtractionParams)]
    lib.loamx_planar_capacity.restype = C.c_size_t
    lib.loamx_planar_capacity.argtypes = [C.POINTER(LidarParams), C.POINTER(FeatureExtractionParams)]
    lib.loamx_extract_features_batch_dev.argtypes = [vp, vp, C.c_size_t, C.POINTER(LidarParams),
                                                     C.POINTER(FeatureExtractionParams), vp, vp, vp, vp, vp, vp]
    lib.loamx_extract_features_batch_dev_f32.argtypes = lib.loamx_extract_features_batch_dev.argtypes
    lib.loamx_register_features_batch_dev.argtypes = [vp, C.c_size_t, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t,
                                                      C.c_size_t, vp, C.POINTER(RegistrationParams), vp]
    lib.loamx_register_scan_pairs_dev.argtypes = [vp, vp, C.c_size_t, C.POINTER(LidarParams),
                                                  C.POINTER(FeatureExtractionParams), C.POINTER(RegistrationParams),
                                                  vp]
    lib.loamx_register_scan_pairs_dev_f32.argtypes = lib.loamx_register_scan_pairs_dev.argtypes
    lib.loamx_register_scan_pairs.argtypes = lib.loamx_register_scan_pairs_dev.argtypes  # (host pointers)
    lib.loamx_register_scan_pairs_f32.argtypes = lib.loamx_register_scan_pairs_dev.argtypes
    lib.loamx_register_scan_sequence_dev.argtypes = [vp, vp, C.c_size_t, C.POINTER(LidarParams),
                                                     C.POINTER(FeatureExtractionParams), C.POINTER(RegistrationParams),
                                                     vp, vp]
    lib.loamx_register_scan_sequence_dev_f32.argtypes = lib.loamx_register_scan_sequence_dev.argtypes
    lib.loamx_register_scan_sequence.argtypes = lib.loamx_register_scan_sequence_dev.argtypes  # (host pointers)
    lib.loamx_register_scan_sequence_f32.argtypes = lib.loamx_register_scan_sequence_dev.argtypes
    lib.loamx_compose_trajectory_dev.argtypes = [vp, vp, C.c_size_t, dp, vp]
    lib.loamx_deskew_scans_dev.argtypes = [vp, vp, C.c_size_t, C.POINTER(LidarParams), vp, C.c_double, vp]
    lib.loamx_deskew_scans_dev_f32.argtypes = lib.loamx_deskew_scans_dev.argtypes
    lib.loamx_deskew_launch_geometry.argtypes = [C.c_size_t, C.c_uint64, C.c_uint64, u32p]
    lib.loamx_ctx_enable_kernel_timing.argtypes = [vp, C.c_int]
    lib.loamx_ctx_reset_kernel_stats.argtypes = [vp]
    lib.loamx_ctx_get_kernel_stats.argtypes = [vp, C.POINTER(KernelStat)]
    lib.loamx_synth_pair_pose.argtypes = [C.c_uint64, C.c_uint64, dp]
    lib.loamx_synth_pair_pose.restype = None
    lib.loamx_synth_scan_host.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, dp]
    lib.loamx_synth_scan_host.restype = None
    lib.loamx_synth_scan_pairs_dev.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_size_t, C.c_uint32, C.c_uint32,
                                               C.c_double, vp]
    lib.loamx_dev_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    lib.loamx_dev_free.argtypes = [vp, vp]
    lib.loamx_copy_to_device.argtypes = [vp, vp, vp, C.c_size_t]
    lib.loamx_copy_to_host.argtypes = [vp, vp, vp, C.c_size_t]
    szp = C.POINTER(C.c_size_t)
    lib.loamx_shard_range.argtypes = [C.c_size_t, C.c_int, C.c_int, szp, szp]
    lib.loamx_shard_range.restype = None
    lib.loamx_comm_get_unique_id.argtypes = [C.c_char_p]
    lib.loamx_comm_create.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, C.POINTER(vp)]
    lib.loamx_comm_wrap.argtypes = [vp, vp, C.POINTER(vp)]
    lib.loamx_comm_destroy.argtypes = [vp]
    lib.loamx_comm_destroy.restype = None
    lib.loamx_comm_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.loamx_gather_results_dev.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, vp]
    lib.loamx_comm_barrier.argtypes = [vp, vp, dp]
    lib.loamx_comm_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.loamx_ctx_extract_counters.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.loamx_fit_lines.argtypes = [vp, dp, C.c_size_t, C.c_size_t, dp, dp]
    lib.loamx_fit_planes.argtypes = [vp, dp, C.c_size_t, C.c_size_t, dp, dp]
    lib.loamx_knn_search.argtypes = [vp, vp, C.c_int, dp, C.c_size_t, C.c_size_t, C.c_double, vp, vp]
    lib.loamx_associate.argtypes = [vp, dp, C.c_size_t, dp, C.c_size_t, dp, C.c_size_t, dp, C.c_size_t, dp,
                                    C.POINTER(RegistrationParams), C.POINTER(AssocDump)]
    lib.loamx_ctx_set_option.argtypes = [vp, C.c_char_p, C.c_int]
    lib.loamx_ctx_get_option.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int)]
    lib.loamx_ctx_last_extract_route.argtypes = [vp, C.POINTER(C.c_uint32)]
    lib.loamx_ctx_last_solve_census.argtypes = [vp, C.c_size_t, C.POINTER(SolveCensusStruct)]
    lib.loamx_ctx_last_assoc_census.argtypes = [vp, C.c_int, C.POINTER(AssocCensusStruct)]
    lib.loamx_ctx_last_assoc_coop_forms.argtypes = [vp, C.c_int, u32p]
    lib.loamx_registration_information.argtypes = [vp, dp, C.c_size_t, dp, C.c_size_t, dp, C.c_size_t, dp, C.c_size_t, dp,
                                                   C.POINTER(RegistrationParams), C.POINTER(RegInformation)]
    lib.loamx_registration_information_indexed.argtypes = [vp, vp, dp, C.c_size_t, dp, C.c_size_t, dp, C.POINTER(RegistrationParams),
                                                           C.POINTER(RegInformation)]
    lib.loamx_registration_information_batch_dev.argtypes = lib.loamx_register_features_batch_dev.argtypes
    lib.loamx_register_scan_pairs_info_dev.argtypes = lib.loamx_register_scan_pairs_dev.argtypes + [vp]
    lib.loamx_register_scan_pairs_info_dev_f32.argtypes = lib.loamx_register_scan_pairs_info_dev.argtypes
    lib.loamx_register_scan_sequence_info_dev.argtypes = lib.loamx_register_scan_sequence_dev.argtypes + [vp]
    lib.loamx_register_scan_sequence_info_dev_f32.argtypes = lib.loamx_register_scan_sequence_info_dev.argtypes
    lib.loamx_default_organize_params.argtypes = [C.POINTER(OrganizeParamsStruct)]
    lib.loamx_default_organize_params.restype = None
    lib.loamx_scan_layout_create.argtypes = [vp, C.POINTER(LidarParams), C.POINTER(OrganizeParamsStruct), C.POINTER(vp)]
    lib.loamx_scan_layout_destroy.argtypes = [vp, vp]
    lib.loamx_scan_layout_destroy.restype = None
    lib.loamx_scan_layout_tables.argtypes = [vp, dp, dp]
    lib.loamx_organize_clouds_dev.argtypes = [vp, vp, vp, C.c_size_t, vp, szp, C.c_size_t, vp, vp, vp]
    lib.loamx_organize_clouds_dev_f32.argtypes = lib.loamx_organize_clouds_dev.argtypes
    lib.loamx_organize_cloud.argtypes = [vp, vp, vp, C.c_size_t, vp, C.c_size_t, vp, vp, vp]
    lib.loamx_organize_cloud_f32.argtypes = lib.loamx_organize_cloud.argtypes
    lib.loamx_default_place_params.argtypes = [C.POINTER(PlaceParamsStruct)]
    lib.loamx_default_place_params.restype = None
    lib.loamx_place_db_create.argtypes = [vp, C.POINTER(PlaceParamsStruct), C.POINTER(vp)]
    lib.loamx_place_db_destroy.argtypes = [vp, vp]
    lib.loamx_place_db_destroy.restype = None
    lib.loamx_place_db_sector_dirs.argtypes = [vp, dp]
    lib.loamx_place_db_size.argtypes = [vp, szp]
    lib.loamx_place_descriptors_dev.argtypes = [vp, vp, vp, C.c_size_t, szp, C.c_size_t, vp]
    lib.loamx_place_descriptors_dev_f32.argtypes = lib.loamx_place_descriptors_dev.argtypes
    lib.loamx_place_db_add_dev.argtypes = [vp, vp, vp, C.c_size_t, u32p]
    lib.loamx_place_db_read.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, vp, vp]
    lib.loamx_place_search_dev.argtypes = [vp, vp, vp, C.c_size_t, vp, C.c_uint32, vp]
    lib.loamx_place_descriptor.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, vp]
    lib.loamx_place_descriptor_f32.argtypes = lib.loamx_place_descriptor.argtypes
    lib.loamx_place_search.argtypes = lib.loamx_place_search_dev.argtypes
    lib.loamx_default_cloud_map_params.argtypes = [C.POINTER(CloudMapParamsStruct)]
    lib.loamx_default_cloud_map_params.restype = None
    lib.loamx_cloud_map_create.argtypes = [vp, C.POINTER(CloudMapParamsStruct), C.c_size_t, C.POINTER(vp)]
    lib.loamx_cloud_map_destroy.argtypes = [vp, vp]
    lib.loamx_cloud_map_destroy.restype = None
    lib.loamx_cloud_map_clear.argtypes = [vp, vp]
    lib.loamx_cloud_map_add_clouds_dev.argtypes = [vp, vp, vp, C.c_size_t, szp, C.c_size_t, vp]
    lib.loamx_cloud_map_add_clouds_dev_f32.argtypes = lib.loamx_cloud_map_add_clouds_dev.argtypes
    lib.loamx_cloud_map_emit_dev.argtypes = [vp, vp, C.c_uint32, vp, vp, vp, C.c_size_t, vp]
    lib.loamx_cloud_map_stats_read.argtypes = [vp, vp, vp]
    lib.loamx_cloud_map_claims_read.argtypes = [vp, vp, C.POINTER(C.c_uint64)]
    lib.loamx_cloud_map_add_cloud.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, vp]
    lib.loamx_cloud_map_add_cloud_f32.argtypes = lib.loamx_cloud_map_add_cloud.argtypes
    lib.loamx_cloud_map_emit.argtypes = [vp, vp, C.c_uint32, vp, vp, vp, C.c_size_t, szp]
    lib.loamx_default_occupancy_params.argtypes = [C.POINTER(OccupancyParamsStruct)]
    lib.loamx_default_occupancy_params.restype = None
    lib.loamx_occupancy_create.argtypes = [vp, C.POINTER(OccupancyParamsStruct), C.c_size_t, C.POINTER(vp)]
    lib.loamx_occupancy_destroy.argtypes = [vp, vp]
    lib.loamx_occupancy_destroy.restype = None
    lib.loamx_occupancy_clear.argtypes = [vp, vp]
    lib.loamx_occupancy_add_clouds_dev.argtypes = [vp, vp, vp, C.c_size_t, szp, C.c_size_t, vp]
    lib.loamx_occupancy_add_clouds_dev_f32.argtypes = lib.loamx_occupancy_add_clouds_dev.argtypes
    lib.loamx_occupancy_query_dev.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, vp, vp]
    lib.loamx_occupancy_query.argtypes = lib.loamx_occupancy_query_dev.argtypes
    lib.loamx_occupancy_box_dev.argtypes = [vp, vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), vp, vp]
    lib.loamx_occupancy_box.argtypes = lib.loamx_occupancy_box_dev.argtypes
    lib.loamx_occupancy_slice_dev.argtypes = [vp, vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), vp]
    lib.loamx_occupancy_slice.argtypes = lib.loamx_occupancy_slice_dev.argtypes
    lib.loamx_default_distance_params.argtypes = [C.POINTER(DistanceParamsStruct)]
    lib.loamx_default_distance_params.restype = None
    for name in ("loamx_occupancy_distance_box", "loamx_occupancy_distance_slice", "loamx_occupancy_distance_box_host",
                 "loamx_occupancy_distance_slice_host"):
        getattr(lib, name).argtypes = [vp, vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(DistanceParamsStruct), vp, vp, vp]
    lib.loamx_default_raycast_params.argtypes = [C.POINTER(RaycastParamsStruct)]
    lib.loamx_default_raycast_params.restype = None
    lib.loamx_occupancy_cast_rays.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_size_t, C.POINTER(RaycastParamsStruct), vp]
    lib.loamx_occupancy_cast_rays_host.argtypes = lib.loamx_occupancy_cast_rays.argtypes
    lib.loamx_occupancy_render_scans.argtypes = [vp, vp, vp, C.c_size_t, vp, C.c_size_t, C.c_double, C.POINTER(RaycastParamsStruct), vp, vp, vp]
    lib.loamx_occupancy_render_scans_host.argtypes = lib.loamx_occupancy_render_scans.argtypes
    lib.loamx_ctx_last_raycast_census.argtypes = [vp, vp]
    lib.loamx_occupancy_stats_read.argtypes = [vp, vp, vp]
    lib.loamx_occupancy_claims_read.argtypes = [vp, vp, C.POINTER(C.c_uint64)]
    lib.loamx_occupancy_add_cloud.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, vp]
    lib.loamx_occupancy_add_cloud_f32.argtypes = lib.loamx_occupancy_add_cloud.argtypes
    lib.loamx_default_surfel_map_params.argtypes = [C.POINTER(SurfelMapParamsStruct)]
    lib.loamx_default_surfel_map_params.restype = None
    lib.loamx_surfel_map_create.argtypes = [vp, C.POINTER(SurfelMapParamsStruct), C.c_size_t, C.POINTER(vp)]
    lib.loamx_surfel_map_destroy.argtypes = [vp, vp]
    lib.loamx_surfel_map_destroy.restype = None
    lib.loamx_surfel_map_clear.argtypes = [vp, vp]
    for name in ("loamx_cloud_map_crop", "loamx_surfel_map_crop", "loamx_occupancy_crop"):
        getattr(lib, name).argtypes = [vp, vp, vp, vp, vp, vp]
    lib.loamx_surfel_map_add_clouds.argtypes = [vp, vp, vp, C.c_size_t, szp, C.c_size_t, vp]
    lib.loamx_surfel_map_add_clouds_f32.argtypes = lib.loamx_surfel_map_add_clouds.argtypes
    lib.loamx_surfel_map_emit.argtypes = [vp, vp, C.c_uint32, vp, vp, vp, C.c_size_t, vp]
    lib.loamx_surfel_map_query.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_uint32, vp, vp, vp]
    lib.loamx_surfel_map_stats_read.argtypes = [vp, vp, vp]
    lib.loamx_surfel_map_claims_read.argtypes = [vp, vp, C.POINTER(C.c_uint64)]
    lib.loamx_surfel_map_add_cloud_host.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, vp]
    lib.loamx_surfel_map_add_cloud_host_f32.argtypes = lib.loamx_surfel_map_add_cloud_host.argtypes
    lib.loamx_surfel_map_emit_host.argtypes = [vp, vp, C.c_uint32, vp, C.c_size_t, szp]
    lib.loamx_default_localize_params.argtypes = [C.POINTER(LocalizeParamsStruct)]
    lib.loamx_default_localize_params.restype = None
    lib.loamx_surfel_localizer_create.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.POINTER(vp)]
    lib.loamx_surfel_localizer_destroy.argtypes = [vp, vp]
    lib.loamx_surfel_localizer_destroy.restype = None
    lib.loamx_surfel_localizer_run.argtypes = [vp, vp, vp, C.c_size_t, szp, C.c_size_t, vp, vp, vp, vp, C.POINTER(LocalizeParamsStruct)]
    lib.loamx_surfel_localizer_run_f32.argtypes = lib.loamx_surfel_localizer_run.argtypes
    lib.loamx_surfel_localizer_run_host.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, vp, C.POINTER(LocalizeParamsStruct), vp, vp]
    lib.loamx_surfel_localizer_run_host_f32.argtypes = lib.loamx_surfel_localizer_run_host.argtypes
    lib.loamx_default_segment_params.argtypes = [C.POINTER(SegmentParamsStruct)]
    lib.loamx_default_segment_params.restype = None
    lib.loamx_segment_constants.argtypes = [C.POINTER(SegmentParamsStruct), dp]
    lib.loamx_segment_scans_dev.argtypes = [vp, vp, C.c_size_t, C.POINTER(LidarParams), C.POINTER(SegmentParamsStruct), vp, vp, vp, vp, vp,
                                            C.c_size_t, vp]
    lib.loamx_segment_scans_dev_f32.argtypes = lib.loamx_segment_scans_dev.argtypes
    lib.loamx_segment_scan.argtypes = [vp, vp, C.POINTER(LidarParams), C.POINTER(SegmentParamsStruct), vp, vp, vp, vp, vp, C.c_size_t, vp]
    lib.loamx_segment_scan_f32.argtypes = lib.loamx_segment_scan.argtypes
    lib.loamx_ctx_last_segment_census.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.loamx_default_visibility_params.argtypes = [C.POINTER(VisibilityParamsStruct)]
    lib.loamx_default_visibility_params.restype = None
    lib.loamx_visibility_votes_dev.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, vp, C.POINTER(VisibilityParamsStruct), C.c_int, vp]
    lib.loamx_visibility_votes_dev_f32.argtypes = lib.loamx_visibility_votes_dev.argtypes
    lib.loamx_visibility_filter_dev.argtypes = [vp, vp, C.c_size_t, C.POINTER(VisibilityParamsStruct), vp, C.c_size_t, vp, vp, vp, C.c_size_t, vp]
    lib.loamx_visibility_votes.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, vp, C.POINTER(VisibilityParamsStruct), vp]
    lib.loamx_visibility_votes_f32.argtypes = lib.loamx_visibility_votes.argtypes
    lib.loamx_ctx_last_visibility_census.argtypes = [vp, C.POINTER(VisibilityCensusStruct)]
    lib.loamx_pgo_default_params.argtypes = [C.POINTER(PgoParamsStruct)]
    lib.loamx_pgo_default_params.restype = None
    lib.loamx_pose_graph_optimize_dev.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_size_t, C.POINTER(PgoParamsStruct), vp]
    lib.loamx_pose_graph_optimize.argtypes = lib.loamx_pose_graph_optimize_dev.argtypes  # (host pointers)
    lib.loamx_pose_graph_linearize.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_double, vp]
    lib.loamx_pose_graph_edges_from_results_dev.argtypes = [vp, vp, vp, C.c_size_t, C.c_uint32, vp]
    _lib = lib
    return lib


class LoamxError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(message)
        self.status = status


DeskewGeometry = collections.namedtuple("DeskewGeometry", "col_blocks shares lines_per_share unroll")


def deskew_launch_geometry(n_scans, scan_lines, points_per_line):
    """The launch loamx_deskew_scans_dev makes for this batch (loamx_deskew_launch_geometry: the launcher's own function):
    column blocks of 256 per scan, shares of the lines, lines per share, lines in flight per thread."""
    v = (C.c_uint32 * 4)()
    rc = load().loamx_deskew_launch_geometry(n_scans, scan_lines, points_per_line, v)
    if rc != OK:
        raise LoamxError(rc, "loamx_deskew_launch_geometry: " + load().loamx_status_string(rc).decode())
    return DeskewGeometry(*(int(x) for x in v))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _pts(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, 3))
    return a


def _scan(a):
    """A scan as an (N,3) array: float32 input stays float32 (FP32-input entry points), anything else is float64."""
    a = np.asarray(a)
    return np.ascontiguousarray(a.reshape(-1, 3)) if a.dtype == np.float32 else _pts(a)


def _xyzp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float if a.dtype == np.float32 else C.c_double))


def synth_pair_pose(seed, pair_id):
    out = np.empty(7)
    load().loamx_synth_pair_pose(seed, pair_id, _dp(out))
    return out


def synth_scan_host(seed, pair_id, which, scan_lines, points_per_line, sigma=0.01):
    out = np.empty((scan_lines * points_per_line, 3))
    load().loamx_synth_scan_host(seed, pair_id, which, scan_lines, points_per_line, sigma, _dp(out))
    return out


COMM_ID_BYTES = 128


def shard_range(total_pairs, world_size, rank):
    """[first, first + count) of `rank`: the partition loamx_gather_results_dev expects (pure host arithmetic)."""
    f, n = C.c_size_t(0), C.c_size_t(0)
    load().loamx_shard_range(total_pairs, world_size, rank, C.byref(f), C.byref(n))
    return f.value, n.value


def comm_unique_id():
    """128-byte RCCL unique id; rank 0 creates it and hands it to every rank (loamx_comm_get_unique_id)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = load().loamx_comm_get_unique_id(buf)
    if rc != OK:
        raise LoamxError(rc, "loamx_comm_get_unique_id: " + load().loamx_status_string(rc).decode())
    return buf.raw


class Comm:
    """RCCL communicator of the multi-GPU batch mode (loamx_comm): one rank per process and GPU."""

    def __init__(self, ctx, unique_id, world_size, rank):
        self.ctx = ctx
        h = C.c_void_p()
        ctx._check(ctx.lib.loamx_comm_create(ctx.h, bytes(unique_id), world_size, rank, C.byref(h)))
        self.h = h

    def info(self):
        w, r, d = C.c_int(0), C.c_int(0), C.c_int(0)
        self.ctx._check(self.ctx.lib.loamx_comm_info(self.h, C.byref(w), C.byref(r), C.byref(d)))
        return dict(world_size=w.value, rank=r.value, device=d.value)

    def gather_results_dev(self, d_local, n_local, total_pairs, d_all):
        """all ranks: d_all[total_pairs] <- every rank's records in pair-id order (asynchronous on the context stream)"""
        self.ctx._check(self.ctx.lib.loamx_gather_results_dev(self.ctx.h, self.h, d_local, n_local, total_pairs, d_all))

    def barrier(self, value=0.0):
        """waits for all ranks; returns the maximum of `value` over the ranks"""
        v = C.c_double(value)
        self.ctx._check(self.ctx.lib.loamx_comm_barrier(self.ctx.h, self.h, C.byref(v)))
        return v.value

    def stats(self):
        """what gather_results_dev / barrier have really enqueued so far (loamx_comm_stats): collectives by kind, and the
        one-rank device-copy shortcuts"""
        v = (C.c_uint64 * 4)()
        self.ctx._check(self.ctx.lib.loamx_comm_stats(self.h, v))
        return dict(ncclAllGather=int(v[0]), ncclBroadcast=int(v[1]), ncclAllReduce=int(v[2]), memcpy=int(v[3]))

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.loamx_comm_destroy(self.h)
            self.h = None


class ScanLayout:
    """The grid an unordered cloud is put into (loamx_scan_layout): lidar.scan_lines x lidar.points_per_line cells, with the
    tables of column and line boundaries on the context's device. close() frees it; the context must still be open."""

    def __init__(self, ctx, lidar, params=None):
        self.ctx, self.params = ctx, params or OrganizeParams()
        self.scan_lines, self.points_per_line = int(lidar.scan_lines), int(lidar.points_per_line)
        st = self.params.struct(self.scan_lines)
        h = C.c_void_p()
        ctx._check(ctx.lib.loamx_scan_layout_create(ctx.h, C.byref(lidar), C.byref(st), C.byref(h)))
        self.h = h

    @property
    def cells(self):
        return self.scan_lines * self.points_per_line

    def tables(self):
        """(col_dirs (W, 2), line_tans (H + 1,)): the bytes the kernels read (loamx_scan_layout_tables)"""
        col, tan = np.empty((self.points_per_line, 2)), np.empty(self.scan_lines + 1)
        self.ctx._check(self.ctx.lib.loamx_scan_layout_tables(self._handle(), _dp(col), _dp(tan)))
        return col, tan

    def _handle(self):
        if not getattr(self, "h", None):
            raise ValueError("the scan layout is closed")
        return self.h

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None):
                self.ctx.lib.loamx_scan_layout_destroy(self.ctx.h, self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _offsets(cloud_offsets, who):
    off = np.ascontiguousarray(cloud_offsets)
    if off.ndim != 1 or off.size < 1 or off.dtype.kind not in "iu":
        raise ValueError(who + ": cloud_offsets is a 1-d integer array of n_clouds + 1 offsets")
    if off.dtype.kind == "i" and (off < 0).any():
        raise ValueError(who + ": negative offset")
    return off.astype(np.uint64)


class PlaceDb:
    """A place-recognition database (loamx_place_db; include/loamx.h, "place recognition"): the parameters, the table of sector
    boundaries and the stored descriptors with their ring keys and column norms, on the context's device. Descriptors are
    (n_rings, n_sectors) uint16 arrays. close() frees it; the context must still be open."""

    def __init__(self, ctx, params=None):
        self.ctx, self.params = ctx, params or PlaceParams()
        st = self.params.struct()
        h = C.c_void_p()
        ctx._check(ctx.lib.loamx_place_db_create(ctx.h, C.byref(st), C.byref(h)))
        self.h = h
        self.n_rings, self.n_sectors = self.params.n_rings, self.params.n_sectors

    @property
    def cells(self):
        return self.n_rings * self.n_sectors

    def _handle(self):
        if not getattr(self, "h", None):
            raise ValueError("the place database is closed")
        return self.h

    def sector_dirs(self):
        """(n_sectors, 2): the sector boundaries as the kernels read them (loamx_place_db_sector_dirs)"""
        d = np.empty((self.n_sectors, 2))
        self.ctx._check(self.ctx.lib.loamx_place_db_sector_dirs(self._handle(), _dp(d)))
        return d

    def size(self):
        n = C.c_size_t(0)
        self.ctx._check(self.ctx.lib.loamx_place_db_size(self._handle(), C.byref(n)))
        return n.value

    def descriptors_dev(self, d_points, point_stride, cloud_offsets, d_desc, f32=False):
        """len(cloud_offsets) - 1 device-resident clouds back to back -> as many descriptors at the device address d_desc
        (loamx_place_descriptors_dev[_f32]). Asynchronous on the context's stream."""
        off = _offsets(cloud_offsets, "descriptors_dev")
        fn = self.ctx.lib.loamx_place_descriptors_dev_f32 if f32 else self.ctx.lib.loamx_place_descriptors_dev
        self.ctx._check(fn(self.ctx.h, self._handle(), d_points or None, int(point_stride), off.ctypes.data_as(C.POINTER(C.c_size_t)),
                           off.size - 1, d_desc or None))

    def descriptor(self, points):
        """One cloud (or organised scan) in host memory, (n, k >= 3) float64 / float32 -> its (n_rings, n_sectors) uint16 descriptor."""
        pts = np.asarray(points)
        if pts.dtype != np.float32:
            pts = np.asarray(pts, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] < 3:
            raise ValueError(f"descriptor: points must be (n, 3) or (n, k >= 3), not {pts.shape}")
        pts = np.ascontiguousarray(pts)
        desc = np.empty((self.n_rings, self.n_sectors), dtype=np.uint16)
        fn = self.ctx.lib.loamx_place_descriptor_f32 if pts.dtype == np.float32 else self.ctx.lib.loamx_place_descriptor
        self.ctx._check(fn(self.ctx.h, self._handle(), pts.ctypes.data, pts.shape[1], pts.shape[0], desc.ctypes.data))
        return desc

    def _descs(self, desc, who):
        d = np.ascontiguousarray(desc, dtype=np.uint16)
        if d.size % self.cells or (d.ndim >= 2 and d.shape[-2:] != (self.n_rings, self.n_sectors) and d.shape[-1] != self.cells):
            raise ValueError(f"{who}: descriptors are (n, {self.n_rings}, {self.n_sectors}) uint16, not {d.shape}")
        return d.reshape(-1, self.n_rings, self.n_sectors)

    def add_dev(self, d_desc, n):
        """appends n descriptors at the device address d_desc; returns the id of the first (loamx_place_db_add_dev)"""
        first = C.c_uint32(0)
        self.ctx._check(self.ctx.lib.loamx_place_db_add_dev(self.ctx.h, self._handle(), d_desc or None, int(n), C.byref(first)))
        return first.value

    def add(self, desc):
        """appends host descriptors, (n_rings, n_sectors) or (n, n_rings, n_sectors); returns the id of the first"""
        d = self._descs(desc, "add")
        if len(d) == 0:
            return self.add_dev(0, 0)
        buf = self.ctx.alloc(d.nbytes)
        try:
            buf.upload(d)
            first = self.add_dev(buf.ptr, len(d))
            self.ctx.synchronize()
            return first
        finally:
            buf.free()

    def read(self, first=0, count=None):
        """(descriptors (count, R, S) uint16, ring keys (count, R) uint32, column norms (count, S) uint64) of stored entries"""
        count = self.size() - first if count is None else count
        desc = np.empty((count, self.n_rings, self.n_sectors), dtype=np.uint16)
        keys, norms = np.empty((count, self.n_rings), dtype=np.uint32), np.empty((count, self.n_sectors), dtype=np.uint64)
        self.ctx._check(self.ctx.lib.loamx_place_db_read(self.ctx.h, self._handle(), first, count, desc.ctypes.data, keys.ctypes.data,
                                                         norms.ctypes.data))
        return desc, keys, norms

    @staticmethod
    def _id_end(id_end, n_queries):
        if id_end is None:
            return None
        e = np.ascontiguousarray(np.broadcast_to(np.asarray(id_end), (n_queries,)))
        if e.dtype.kind not in "iu" or (e.size and (e.min() < 0 or e.max() > 0xFFFFFFFF)):
            raise ValueError("search: id_end holds integers in 0 .. 2^32 - 1")
        return e.astype(np.uint32)

    def search_dev(self, d_query_desc, n_queries, num_candidates, d_out, id_end=None):
        """n_queries descriptors at the device address d_query_desc -> n_queries x num_candidates PLACE_MATCH_DTYPE records at
        d_out (loamx_place_search_dev). id_end: None, one integer or one per query (host). Asynchronous."""
        e = self._id_end(id_end, n_queries)
        self.ctx._check(self.ctx.lib.loamx_place_search_dev(self.ctx.h, self._handle(), d_query_desc or None, int(n_queries),
                                                            e.ctypes.data if e is not None else None, int(num_candidates), d_out or None))

    def search(self, desc, num_candidates, id_end=None):
        """host descriptors (R, S) or (n, R, S) -> (n, num_candidates) PLACE_MATCH_DTYPE records, ascending by (distance, id)"""
        d = self._descs(desc, "search")
        e = self._id_end(id_end, len(d))
        out = np.empty((len(d), int(num_candidates)), dtype=PLACE_MATCH_DTYPE)
        self.ctx._check(self.ctx.lib.loamx_place_search(self.ctx.h, self._handle(), d.ctypes.data, len(d),
                                                        e.ctypes.data if e is not None else None, int(num_candidates), out.ctypes.data))
        return out

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None):
                self.ctx.lib.loamx_place_db_destroy(self.ctx.h, self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _VoxelMap:
    """What CloudMap, OccupancyMap and SurfelMap share: the handle, clear, the two forms of an add, claims and close. A subclass names the
    prefix of its C entry points, its parameters class and itself (the error texts)."""
    _PREFIX = _PARAMS = _NAME = None

    def __init__(self, ctx, params=None, max_voxels=1 << 20):
        self.ctx, self.params = ctx, params or self._PARAMS()
        max_voxels = int(max_voxels)
        if max_voxels < 0:
            raise ValueError(f"{self._NAME.replace(' ', '_')}: max_voxels is negative")
        st = self.params.struct()
        h = C.c_void_p()
        ctx._check(self._fn("create")(ctx.h, C.byref(st), max_voxels, C.byref(h)))
        self.h, self.max_voxels = h, max_voxels

    def _fn(self, name):
        return getattr(self.ctx.lib, self._PREFIX + name)

    def _handle(self):
        if not getattr(self, "h", None):
            raise ValueError(f"the {self._NAME} is closed")
        return self.h

    def clear(self):
        """an empty map again (loamx_cloud_map_clear / loamx_occupancy_clear). Asynchronous."""
        self.ctx._check(self._fn("clear")(self.ctx.h, self._handle()))

    @staticmethod
    def _crop_bounds(lo, hi, what):
        lo, hi = np.asarray(lo), np.asarray(hi)
        if lo.shape != (3,) or hi.shape != (3,) or lo.dtype.kind not in "fiu" or hi.dtype.kind not in "fiu":
            raise ValueError(f"{what}: lo and hi are three numbers each")
        return np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)

    def crop_dev(self, lo, hi, d_pose=0, d_counts_out=0):
        """the voxels outside the box centre + [lo, hi] leave the map (include/loamx.h, "map window"); the centre is the translation
        of the pose at the device address d_pose (7 doubles), or (0, 0, 0) for 0; lo, hi: host values, three each; d_counts_out: a
        device address of four uint32 {kept, removed, skipped, 0}, or 0 (loamx_cloud_map_crop / loamx_surfel_map_crop /
        loamx_occupancy_crop). Asynchronous; the handle's first crop allocates its staging."""
        lo, hi = self._crop_bounds(lo, hi, "crop_dev")
        self.ctx._check(self._fn("crop")(self.ctx.h, self._handle(), d_pose or None, lo.ctypes.data, hi.ctypes.data, d_counts_out or None))

    def crop(self, lo, hi, center=None):
        """crop_dev with a host centre (three numbers, None = the origin) folded into lo and hi on the host, which gives the same
        bytes as the same centre in a device pose -> (kept, removed); synchronises"""
        lo, hi = self._crop_bounds(lo, hi, "crop")
        if center is not None:
            c = np.asarray(center)
            if c.shape != (3,) or c.dtype.kind not in "fiu":
                raise ValueError("crop: center is three numbers")
            c = c.astype(np.float64)
            if not np.isfinite(c).all():
                raise ValueError("crop: center is not finite")
            lo, hi = c + lo, c + hi
        buf = self.ctx.alloc(16)
        try:
            self.crop_dev(lo, hi, 0, buf.ptr)
            self.ctx.synchronize()
            counts = buf.download(np.uint32, 4)
        finally:
            buf.free()
        return int(counts[0]), int(counts[1])

    def add_clouds_dev(self, d_points, point_stride, cloud_offsets, d_poses=0, f32=False):
        """len(cloud_offsets) - 1 device-resident clouds back to back, cloud c at the pose d_poses[c] (a device address of
        n_clouds x 7 doubles, or 0 = no transform) (loamx_cloud_map_add_clouds_dev[_f32] / loamx_occupancy_add_clouds_dev[_f32]).
        Asynchronous."""
        off = _offsets(cloud_offsets, "add_clouds_dev")
        if int(point_stride) < 0:
            raise ValueError("add_clouds_dev: point_stride is negative")
        fn = self._fn("add_clouds_dev_f32" if f32 else "add_clouds_dev")
        self.ctx._check(fn(self.ctx.h, self._handle(), d_points or None, int(point_stride), off.ctypes.data_as(C.POINTER(C.c_size_t)),
                           off.size - 1, d_poses or None))

    def add_cloud(self, points, pose=None):
        """One cloud (or organised scan) in host memory, (n, k >= 3) float64 / float32, at a host pose7 or None (no transform)."""
        pts = np.asarray(points)
        if pts.dtype != np.float32:
            pts = np.asarray(pts, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] < 3:
            raise ValueError(f"add_cloud: points must be (n, 3) or (n, k >= 3), not {pts.shape}")
        pts = np.ascontiguousarray(pts)
        p = None
        if pose is not None:
            p = np.ascontiguousarray(pose, dtype=np.float64)
            if p.shape != (7,):
                raise ValueError(f"add_cloud: a pose is 7 numbers (qx qy qz qw tx ty tz), not {p.shape}")
        fn = self._fn("add_cloud_f32" if pts.dtype == np.float32 else "add_cloud")
        self.ctx._check(fn(self.ctx.h, self._handle(), pts.ctypes.data, pts.shape[1], pts.shape[0], None if p is None else p.ctypes.data))

    def claims(self):
        """probes begun by the map's add kernel since the last clear: one per used point (cloud map) or per hit and per pass
        (occupancy map) in the plain form, one per run of a wavefront with run combining (loamx_cloud_map_claims_read /
        loamx_occupancy_claims_read; synchronises)"""
        n = C.c_uint64(0)
        self.ctx._check(self._fn("claims_read")(self.ctx.h, self._handle(), C.byref(n)))
        return n.value

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None):
                self._fn("destroy")(self.ctx.h, self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CloudMap(_VoxelMap):
    """A cloud map (loamx_cloud_map; include/loamx.h, "cloud map"): posed clouds accumulated on a voxel grid as integer sums, one
    centroid per voxel, the voxels in order of first appearance; on the context's device. close() frees it; the context must
    still be open."""
    _PREFIX, _PARAMS, _NAME = "loamx_cloud_map_", CloudMapParams, "cloud map"

    def emit_dev(self, d_xyz_out, capacity, d_n_out, min_points=1, d_count_out=0, d_first_out=0):
        """the centroids of the voxels with count >= min_points in list order, at most `capacity`, to device addresses; the
        number that qualify to d_n_out (loamx_cloud_map_emit_dev). Asynchronous."""
        if int(capacity) < 0 or not 0 <= int(min_points) <= 0xFFFFFFFF:
            raise ValueError("emit_dev: capacity is negative or min_points does not fit 32 bits")
        self.ctx._check(self.ctx.lib.loamx_cloud_map_emit_dev(self.ctx.h, self._handle(), int(min_points), d_xyz_out or None, d_count_out or None,
                                                              d_first_out or None, int(capacity), d_n_out or None))

    def emit(self, min_points=1, capacity=None):
        """(xyz (m, 3) float64, count (m,) uint32, first (m,) uint32, n): m = min(n, capacity) voxels in list order, n the
        number that qualify; capacity None: room for every voxel the map can hold."""
        capacity = self.max_voxels if capacity is None else int(capacity)
        if capacity < 0 or not 0 <= int(min_points) <= 0xFFFFFFFF:
            raise ValueError("emit: capacity is negative or min_points does not fit 32 bits")
        room = min(capacity, self.max_voxels)
        xyz, cnt, first = np.empty((room, 3)), np.empty(room, dtype=np.uint32), np.empty(room, dtype=np.uint32)
        n = C.c_size_t(0)
        self.ctx._check(self.ctx.lib.loamx_cloud_map_emit(self.ctx.h, self._handle(), int(min_points), xyz.ctypes.data, cnt.ctypes.data,
                                                          first.ctypes.data, room, C.byref(n)))
        m = min(n.value, room)
        return xyz[:m], cnt[:m], first[:m], n.value

    def stats(self):
        """one CLOUD_MAP_STATS_DTYPE record (loamx_cloud_map_stats_read; synchronises)"""
        st = np.zeros(1, dtype=CLOUD_MAP_STATS_DTYPE)
        self.ctx._check(self.ctx.lib.loamx_cloud_map_stats_read(self.ctx.h, self._handle(), st.ctypes.data))
        return st[0]


def _box_args(vmin, dims, what):
    """(int32[3], uint32[3]) of a voxel box"""
    v, d = np.asarray(vmin), np.asarray(dims)
    if v.shape != (3,) or d.shape != (3,) or v.dtype.kind not in "iu" or d.dtype.kind not in "iu":
        raise ValueError(f"{what}: vmin and dims are three integers each")
    if (np.abs(v.astype(np.int64)) > 0x7FFFFFFF).any() or (d.astype(np.int64) < 0).any() or (d.astype(np.int64) > 0xFFFFFFFF).any():
        raise ValueError(f"{what}: vmin does not fit int32 or dims does not fit uint32")
    return np.ascontiguousarray(v, dtype=np.int32), np.ascontiguousarray(d, dtype=np.uint32)


class OccupancyMap(_VoxelMap):
    """An occupancy map (loamx_occupancy_map; include/loamx.h, "occupancy map"): every beam of posed clouds walked through a voxel
    grid, two integer counts per voxel (hits, passes), read back as free / occupied / unknown per point, per voxel of a dense
    box or per column of a 2-D slice; on the context's device. close() frees it; the context must still be open."""
    _PREFIX, _PARAMS, _NAME = "loamx_occupancy_", OccupancyParams, "occupancy map"

    def query_dev(self, d_points, point_stride, n, d_counts_out=0, d_state_out=0):
        """counts (uint32 [n][2]: hits, passes) and state (uint8 [n]) of the voxels of n device-resident points (double), to
        device addresses, either 0 = not wanted (loamx_occupancy_query_dev). Asynchronous."""
        if int(point_stride) < 0 or int(n) < 0:
            raise ValueError("query_dev: point_stride or n is negative")
        self.ctx._check(self.ctx.lib.loamx_occupancy_query_dev(self.ctx.h, self._handle(), d_points or None, int(point_stride), int(n),
                                                               d_counts_out or None, d_state_out or None))

    def query(self, points):
        """host points (n, k >= 3) -> (counts (n, 2) uint32, state (n,) uint8)"""
        pts = np.ascontiguousarray(points, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] < 3:
            raise ValueError(f"query: points must be (n, 3) or (n, k >= 3), not {pts.shape}")
        counts, state = np.zeros((len(pts), 2), dtype=np.uint32), np.zeros(len(pts), dtype=np.uint8)
        self.ctx._check(self.ctx.lib.loamx_occupancy_query(self.ctx.h, self._handle(), pts.ctypes.data, pts.shape[1], len(pts), counts.ctypes.data,
                                                           state.ctypes.data))
        return counts, state

    def box_dev(self, vmin, dims, d_counts_out=0, d_state_out=0):
        """the voxels vmin .. vmin + dims - 1, x fastest, to device addresses, either 0 = not wanted (loamx_occupancy_box_dev).
        Asynchronous."""
        v, d = _box_args(vmin, dims, "box_dev")
        self.ctx._check(self.ctx.lib.loamx_occupancy_box_dev(self.ctx.h, self._handle(), v.ctypes.data_as(C.POINTER(C.c_int32)),
                                                             d.ctypes.data_as(C.POINTER(C.c_uint32)), d_counts_out or None, d_state_out or None))

    def box(self, vmin, dims):
        """(counts (dz, dy, dx, 2) uint32, state (dz, dy, dx) uint8) of the box"""
        v, d = _box_args(vmin, dims, "box")
        shape = (int(d[2]), int(d[1]), int(d[0]))
        counts, state = np.zeros(shape + (2,), dtype=np.uint32), np.zeros(shape, dtype=np.uint8)
        self.ctx._check(self.ctx.lib.loamx_occupancy_box(self.ctx.h, self._handle(), v.ctypes.data_as(C.POINTER(C.c_int32)),
                                                         d.ctypes.data_as(C.POINTER(C.c_uint32)), counts.ctypes.data, state.ctypes.data))
        return counts, state

    def slice_dev(self, vmin, dims, d_grid_out):
        """the 2-D grid (uint8 [dims[1]][dims[0]]) of the box's columns to a device address (loamx_occupancy_slice_dev). Asynchronous."""
        v, d = _box_args(vmin, dims, "slice_dev")
        self.ctx._check(self.ctx.lib.loamx_occupancy_slice_dev(self.ctx.h, self._handle(), v.ctypes.data_as(C.POINTER(C.c_int32)),
                                                               d.ctypes.data_as(C.POINTER(C.c_uint32)), d_grid_out or None))

    def slice(self, vmin, dims):
        """(dy, dx) uint8: OCC_OCCUPIED where any level of the column is occupied, otherwise OCC_FREE where any is free"""
        v, d = _box_args(vmin, dims, "slice")
        grid = np.zeros((int(d[1]), int(d[0])), dtype=np.uint8)
        self.ctx._check(self.ctx.lib.loamx_occupancy_slice(self.ctx.h, self._handle(), v.ctypes.data_as(C.POINTER(C.c_int32)),
                                                           d.ctypes.data_as(C.POINTER(C.c_uint32)), grid.ctypes.data))
        return grid

    def _distance_dev(self, name, vmin, dims, params, d_d2_out, d_offset_out, d_metres_out):
        v, d = _box_args(vmin, dims, name)
        st = (params or DistanceParams()).struct()
        self.ctx._check(getattr(self.ctx.lib, "loamx_occupancy_" + name)(
            self.ctx.h, self._handle(), v.ctypes.data_as(C.POINTER(C.c_int32)), d.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(st),
            d_d2_out or None, d_offset_out or None, d_metres_out or None))

    def distance_box_dev(self, vmin, dims, params=None, d_d2_out=0, d_offset_out=0, d_metres_out=0):
        """the distance field of the box (include/loamx.h, "occupancy distance field") to device addresses, each 0 = not wanted:
        squared distances in voxels (uint16 [n], DIST_FAR beyond the cap), offsets to the nearest obstacle (int16 [n][3]) and metres
        (float32 [n]), in the layout of box_dev (loamx_occupancy_distance_box). Asynchronous."""
        self._distance_dev("distance_box", vmin, dims, params, d_d2_out, d_offset_out, d_metres_out)

    def distance_slice_dev(self, vmin, dims, params=None, d_d2_out=0, d_offset_out=0, d_metres_out=0):
        """the 2-D distance field of the box's columns to device addresses, each 0 = not wanted: uint16 [dims[1]][dims[0]], int16
        [.][2], float32 (loamx_occupancy_distance_slice). Asynchronous."""
        self._distance_dev("distance_slice", vmin, dims, params, d_d2_out, d_offset_out, d_metres_out)

    def _distance_host(self, name, vmin, dims, params, shape, axes):
        v, d = _box_args(vmin, dims, name)
        st = (params or DistanceParams()).struct()
        d2, offset, metres = np.zeros(shape, dtype=np.uint16), np.zeros(shape + (axes,), dtype=np.int16), np.zeros(shape, dtype=np.float32)
        self.ctx._check(getattr(self.ctx.lib, "loamx_occupancy_" + name + "_host")(
            self.ctx.h, self._handle(), v.ctypes.data_as(C.POINTER(C.c_int32)), d.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(st),
            d2.ctypes.data, offset.ctypes.data, metres.ctypes.data))
        return d2, offset, metres

    def distance_box(self, vmin, dims, params=None):
        """(d2 (dz, dy, dx) uint16, offset (dz, dy, dx, 3) int16, metres (dz, dy, dx) float32) of the box"""
        return self._distance_host("distance_box", vmin, dims, params, (int(dims[2]), int(dims[1]), int(dims[0])), 3)

    def distance_slice(self, vmin, dims, params=None):
        """(d2 (dy, dx) uint16, offset (dy, dx, 2) int16, metres (dy, dx) float32) of the box's columns"""
        return self._distance_host("distance_slice", vmin, dims, params, (int(dims[1]), int(dims[0])), 2)

    def cast_rays_dev(self, d_origins, d_ends, stride, n, d_records_out, params=None):
        """n device-resident segments (double, map frame, `stride` doubles apart) cast through the map (include/loamx.h, "occupancy
        ray casting"): one RAY_RECORD_DTYPE record each to a device address (loamx_occupancy_cast_rays). Asynchronous."""
        if int(stride) < 0 or int(n) < 0:
            raise ValueError("cast_rays_dev: stride or n is negative")
        st = (params or RaycastParams()).struct()
        self.ctx._check(self.ctx.lib.loamx_occupancy_cast_rays(self.ctx.h, self._handle(), d_origins or None, d_ends or None, int(stride), int(n),
                                                               C.byref(st), d_records_out or None))

    def cast_rays(self, origins, ends, params=None):
        """host segments origins -> ends, (n, k >= 3) each with the same k -> (n,) RAY_RECORD_DTYPE records"""
        o, e = np.ascontiguousarray(origins, dtype=np.float64), np.ascontiguousarray(ends, dtype=np.float64)
        if o.ndim != 2 or o.shape[1] < 3 or o.shape != e.shape:
            raise ValueError(f"cast_rays: origins and ends must both be (n, 3) or (n, k >= 3), not {o.shape} and {e.shape}")
        st = (params or RaycastParams()).struct()
        out = np.zeros(len(o), dtype=RAY_RECORD_DTYPE)
        self.ctx._check(self.ctx.lib.loamx_occupancy_cast_rays_host(self.ctx.h, self._handle(), o.ctypes.data, e.ctypes.data, o.shape[1], len(o),
                                                                    C.byref(st), out.ctypes.data))
        return out

    def render_scans_dev(self, d_dirs, n_beams, d_poses, n_poses, max_range, params=None, d_scans_out=0, d_ranges_out=0, d_records_out=0):
        """the scans the map predicts at n_poses device-resident poses (n_poses x 7) for n_beams unit beam directions (n_beams x 3,
        sensor frame, cell order: beam_directions) to device addresses, each 0 = not wanted: points (double [n_poses][n_beams][3],
        (0, 0, 0) where nothing is hit), ranges (double) and records (loamx_occupancy_render_scans). Asynchronous."""
        if int(n_beams) < 0 or int(n_poses) < 0:
            raise ValueError("render_scans_dev: n_beams or n_poses is negative")
        st = (params or RaycastParams()).struct()
        self.ctx._check(self.ctx.lib.loamx_occupancy_render_scans(self.ctx.h, self._handle(), d_dirs or None, int(n_beams), d_poses or None, int(n_poses),
                                                                  float(max_range), C.byref(st), d_scans_out or None, d_ranges_out or None,
                                                                  d_records_out or None))

    def render_scans(self, dirs, poses, max_range, params=None, scans=True, ranges=True, records=True):
        """host beam directions (n_beams, 3) and poses (n_poses, 7) -> (scans (n_poses, n_beams, 3), ranges (n_poses, n_beams),
        records (n_poses, n_beams) RAY_RECORD_DTYPE); an output that is not wanted is None"""
        d, p = np.ascontiguousarray(dirs, dtype=np.float64), np.ascontiguousarray(poses, dtype=np.float64)
        if d.ndim != 2 or d.shape[1] != 3 or p.ndim != 2 or p.shape[1] != 7:
            raise ValueError(f"render_scans: dirs must be (n_beams, 3) and poses (n_poses, 7), not {d.shape} and {p.shape}")
        st = (params or RaycastParams()).struct()
        shape = (len(p), len(d))
        out_s = np.zeros(shape + (3,), dtype=np.float64) if scans else None
        out_r = np.zeros(shape, dtype=np.float64) if ranges else None
        out_k = np.zeros(shape, dtype=RAY_RECORD_DTYPE) if records else None
        self.ctx._check(self.ctx.lib.loamx_occupancy_render_scans_host(
            self.ctx.h, self._handle(), d.ctypes.data, len(d), p.ctypes.data, len(p), float(max_range), C.byref(st),
            out_s.ctypes.data if scans else None, out_r.ctypes.data if ranges else None, out_k.ctypes.data if records else None))
        return out_s, out_r, out_k

    def stats(self):
        """one OCCUPANCY_STATS_DTYPE record (loamx_occupancy_stats_read; synchronises)"""
        st = np.zeros(1, dtype=OCCUPANCY_STATS_DTYPE)
        self.ctx._check(self.ctx.lib.loamx_occupancy_stats_read(self.ctx.h, self._handle(), st.ctypes.data))
        return st[0]


class SurfelMap(_VoxelMap):
    """A surfel map (loamx_surfel_map; include/loamx.h, "surfel map"): posed clouds accumulated on a voxel grid as integer first
    and second moments and a view sum; per voxel the mean, the covariance, its eigenvalues and the normal turned towards the sensor,
    the voxels in order of first appearance; on the context's device. close() frees it; the context must still be open."""
    _PREFIX, _PARAMS, _NAME = "loamx_surfel_map_", SurfelMapParams, "surfel map"
    # on this handle the C names without a suffix are the device forms
    _C_NAMES = {"add_clouds_dev": "add_clouds", "add_clouds_dev_f32": "add_clouds_f32", "add_cloud": "add_cloud_host",
                "add_cloud_f32": "add_cloud_host_f32"}

    def _fn(self, name):
        return getattr(self.ctx.lib, self._PREFIX + self._C_NAMES.get(name, name))

    def emit_dev(self, capacity, d_n_out, min_points=1, d_out=0, d_xyz_out=0, d_normal_out=0):
        """the voxels with count >= min_points in list order, at most `capacity`, to device addresses: SURFEL_DTYPE records, the
        means and the normals (capacity x 3 doubles each), any of them 0 = not wanted; the number that qualify to d_n_out
        (loamx_surfel_map_emit). Asynchronous."""
        if int(capacity) < 0 or not 0 <= int(min_points) <= 0xFFFFFFFF:
            raise ValueError("emit_dev: capacity is negative or min_points does not fit 32 bits")
        self.ctx._check(self.ctx.lib.loamx_surfel_map_emit(self.ctx.h, self._handle(), int(min_points), d_out or None, d_xyz_out or None,
                                                           d_normal_out or None, int(capacity), d_n_out or None))

    def emit(self, min_points=1, capacity=None):
        """(records (m,) SURFEL_DTYPE, n): m = min(n, capacity) voxels in list order, n the number that qualify; capacity None:
        room for every voxel the map can hold (loamx_surfel_map_emit_host; synchronises)."""
        capacity = self.max_voxels if capacity is None else int(capacity)
        if capacity < 0 or not 0 <= int(min_points) <= 0xFFFFFFFF:
            raise ValueError("emit: capacity is negative or min_points does not fit 32 bits")
        room = min(capacity, self.max_voxels)
        out = np.zeros(room, dtype=SURFEL_DTYPE)
        n = C.c_size_t(0)
        self.ctx._check(self.ctx.lib.loamx_surfel_map_emit_host(self.ctx.h, self._handle(), int(min_points), out.ctypes.data, room, C.byref(n)))
        return out[:min(n.value, room)], n.value

    def query_dev(self, d_points, point_stride, n, min_points=1, d_out=0, d_distance_out=0, d_count_out=0):
        """per device-resident point (double): the record of its voxel, the signed distance to its plane and the voxel's count, to
        device addresses, any of them 0 = not wanted (loamx_surfel_map_query). Asynchronous."""
        if int(point_stride) < 0 or int(n) < 0 or not 0 <= int(min_points) <= 0xFFFFFFFF:
            raise ValueError("query_dev: point_stride or n is negative, or min_points does not fit 32 bits")
        self.ctx._check(self.ctx.lib.loamx_surfel_map_query(self.ctx.h, self._handle(), d_points or None, int(point_stride), int(n), int(min_points),
                                                            d_out or None, d_distance_out or None, d_count_out or None))

    def query(self, points, min_points=1):
        """host points (n, k >= 3) -> (records (n,) SURFEL_DTYPE, distance (n,) float64, count (n,) uint32); synchronises"""
        pts = np.ascontiguousarray(points, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] < 3:
            raise ValueError(f"query: points must be (n, 3) or (n, k >= 3), not {pts.shape}")
        n = len(pts)
        rec, dist, cnt = np.zeros(n, dtype=SURFEL_DTYPE), np.zeros(n), np.zeros(n, dtype=np.uint32)
        if n == 0:
            return rec, dist, cnt
        bufs = [self.ctx.alloc(pts.nbytes), self.ctx.alloc(rec.nbytes), self.ctx.alloc(dist.nbytes), self.ctx.alloc(cnt.nbytes)]
        try:
            bufs[0].upload(pts)
            self.query_dev(bufs[0].ptr, pts.shape[1], n, min_points, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr)
            self.ctx.synchronize()
            rec, dist, cnt = bufs[1].download(SURFEL_DTYPE, n), bufs[2].download(np.float64, n), bufs[3].download(np.uint32, n)
        finally:
            for b in bufs:
                b.free()
        return rec, dist, cnt

    def stats(self):
        """one SURFEL_MAP_STATS_DTYPE record (loamx_surfel_map_stats_read; synchronises)"""
        st = np.zeros(1, dtype=SURFEL_MAP_STATS_DTYPE)
        self.ctx._check(self.ctx.lib.loamx_surfel_map_stats_read(self.ctx.h, self._handle(), st.ctypes.data))
        return st[0]

    def localizer(self, max_clouds=1, max_points=1 << 20):
        """a SurfelLocalizer on this map for calls of at most max_clouds clouds and max_points points (loamx_surfel_localizer_create)"""
        return SurfelLocalizer(self, max_clouds, max_points)


class SurfelLocalizer:
    """Scan-to-map localisation on a surfel map (loamx_surfel_localizer; include/loamx.h, "surfel localisation"): point-to-plane
    Gauss-Newton against the voxels' fitted planes, solved on the device. close() frees it, before its map is closed."""

    def __init__(self, surfel_map, max_clouds, max_points):
        max_clouds, max_points = int(max_clouds), int(max_points)
        if max_clouds < 0 or max_points < 0:
            raise ValueError("localizer: max_clouds or max_points is negative")
        self.map, self.ctx, self.max_clouds, self.max_points = surfel_map, surfel_map.ctx, max_clouds, max_points
        h = C.c_void_p()
        self.ctx._check(self.ctx.lib.loamx_surfel_localizer_create(self.ctx.h, surfel_map._handle(), max_clouds, max_points, C.byref(h)))
        self.h = h

    def _handle(self):
        if not getattr(self, "h", None):
            raise ValueError("the localizer is closed")
        return self.h

    def run_dev(self, d_points, point_stride, cloud_offsets, d_poses_in, d_poses_out, d_results, d_info=0, params=None, f32=False):
        """len(cloud_offsets) - 1 device-resident clouds from their device poses (n_clouds x 7 doubles); the poses, the
        LOCALIZE_RESULT_DTYPE records and (d_info != 0) the INFORMATION_DTYPE records to device addresses; d_poses_out may be
        d_poses_in (loamx_surfel_localizer_run[_f32]). Asynchronous."""
        off = _offsets(cloud_offsets, "run_dev")
        if int(point_stride) < 0:
            raise ValueError("run_dev: point_stride is negative")
        st = (params or LocalizeParams()).struct()
        fn = self.ctx.lib.loamx_surfel_localizer_run_f32 if f32 else self.ctx.lib.loamx_surfel_localizer_run
        self.ctx._check(fn(self.ctx.h, self._handle(), d_points or None, int(point_stride), off.ctypes.data_as(C.POINTER(C.c_size_t)), off.size - 1,
                           d_poses_in or None, d_poses_out or None, d_results or None, d_info or None, C.byref(st)))

    def run(self, points, pose, params=None, information=True):
        """One cloud in host memory, (n, k >= 3) float64 / float32, from a host pose7 -> (pose (7,), one LOCALIZE_RESULT_DTYPE record,
        one INFORMATION_DTYPE record or None) (loamx_surfel_localizer_run_host[_f32]; synchronises)."""
        pts = np.asarray(points)
        if pts.dtype != np.float32:
            pts = np.asarray(pts, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] < 3:
            raise ValueError(f"run: points must be (n, 3) or (n, k >= 3), not {pts.shape}")
        pts = np.ascontiguousarray(pts)
        p = np.ascontiguousarray(pose, dtype=np.float64)
        if p.shape != (7,):
            raise ValueError(f"run: a pose is 7 numbers (qx qy qz qw tx ty tz), not {p.shape}")
        st = (params or LocalizeParams()).struct()
        res, info = np.zeros(1, dtype=LOCALIZE_RESULT_DTYPE), np.zeros(1, dtype=INFORMATION_DTYPE)
        fn = self.ctx.lib.loamx_surfel_localizer_run_host_f32 if pts.dtype == np.float32 else self.ctx.lib.loamx_surfel_localizer_run_host
        self.ctx._check(fn(self.ctx.h, self._handle(), pts.ctypes.data, pts.shape[1], pts.shape[0], p.ctypes.data, C.byref(st), res.ctypes.data,
                           info.ctypes.data if information else None))
        return res[0]["pose"].copy(), res[0], (info[0] if information else None)

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None):
                self.ctx.lib.loamx_surfel_localizer_destroy(self.ctx.h, self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceBuffer:
    """Raw device allocation owned by a Context (for hosts that do not use torch tensors)."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, nbytes
        p = C.c_void_p()
        ctx._check(ctx.lib.loamx_dev_alloc(ctx.h, nbytes, C.byref(p)))
        self.ptr = p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.ctx._check(self.ctx.lib.loamx_copy_to_device(self.ctx.h, self.ptr, arr.ctypes.data, arr.nbytes))
        return self

    def download(self, dtype, count):
        out = np.empty(count, dtype=dtype)
        assert out.nbytes <= self.nbytes
        self.ctx._check(self.ctx.lib.loamx_copy_to_host(self.ctx.h, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            self.ctx.lib.loamx_dev_free(self.ctx.h, self.ptr)
            self.ptr = None


class Context:
    """One device + stream + workspace (loamx_ctx)."""

    def __init__(self, device=0):
        self.lib = load()
        h = C.c_void_p()
        rc = self.lib.loamx_ctx_create(device, C.byref(h))
        if rc != OK:
            raise LoamxError(rc, "loamx_ctx_create: " + self.lib.loamx_status_string(rc).decode() +
                             " (libloamx has no CPU fallback)")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.loamx_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != OK:
            msg = self.lib.loamx_last_error(self.h).decode() or self.lib.loamx_status_string(rc).decode()
            raise LoamxError(rc, msg)

    def set_stream(self, hip_stream_handle):
        self._check(self.lib.loamx_ctx_set_stream(self.h, hip_stream_handle))

    def synchronize(self):
        self._check(self.lib.loamx_ctx_synchronize(self.h))

    def set_option(self, name, value=1):
        """debug / measurement switch of this context (include/loamx.h: loamx_ctx_set_option)"""
        self._check(self.lib.loamx_ctx_set_option(self.h, name.encode(), int(value)))

    def get_option(self, name):
        v = C.c_int(0)
        self._check(self.lib.loamx_ctx_get_option(self.h, name.encode(), C.byref(v)))
        return v.value

    def extract_counters(self):
        """(scan lines replayed in the reference's tie order, give-up fallbacks of the fused compaction), cumulative"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.loamx_ctx_extract_counters(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_extract_route(self):
        """which kernels the last extraction on this context took (include/loamx.h: LOAMX_ROUTE_*), as an ExtractRoute"""
        v = C.c_uint32(0)
        self._check(self.lib.loamx_ctx_last_extract_route(self.h, C.byref(v)))
        return ExtractRoute(v.value)

    def last_solve_census(self, pair=0):
        """what the solve kernels of the last registration on this context worked on for `pair` (include/loamx.h:
        loamx_ctx_last_solve_census), as a SolveCensus; tile_counts = the listed plane records of every live moment tile"""
        v = SolveCensusStruct()
        self._check(self.lib.loamx_ctx_last_solve_census(self.h, pair, C.byref(v)))  # (no array: the number of live tiles)
        counts = np.zeros(max(1, v.live_tiles), dtype=np.uint32)
        v.tile_counts, v.tile_counts_cap = counts.ctypes.data_as(C.POINTER(C.c_uint32)), v.live_tiles
        self._check(self.lib.loamx_ctx_last_solve_census(self.h, pair, C.byref(v)))
        return SolveCensus(v.iterations, v.termination, v.use_moments, v.mom_ref_on, np.array(list(v.mom_ref)), v.tiles, v.live_tiles,
                           v.edge_stride, v.planar_stride, v.n_se, v.n_sp, v.walk, v.listed_total, v.s0max, v.v2max, v.sweep_chunk,
                           v.edge_cache, v.list_cache, v.flat_cache, counts[:v.live_tiles].copy())

    def last_assoc_coop_forms(self, kind):
        """(entries a row of lanes took, entries a whole wavefront took) in the cooperative leftover kernel of the last associate()
        on this context, as the kernel counted them (include/loamx.h: loamx_ctx_last_assoc_coop_forms)"""
        kind = {"edge": 0, "plane": 1}.get(kind, kind)
        out = (C.c_uint32 * 2)()
        self._check(self.lib.loamx_ctx_last_assoc_coop_forms(self.h, kind, out))
        return int(out[0]), int(out[1])

    def last_assoc_census(self, kind):
        """the route census of the last associate() on this context for one feature kind (0 / "edge", 1 / "plane"; include/loamx.h:
        loamx_ctx_last_assoc_census), as an AssocCensus with the per-entry arrays of the kind's queue"""
        kind = {"edge": 0, "plane": 1}.get(kind, kind)
        v = AssocCensusStruct()
        self._check(self.lib.loamx_ctx_last_assoc_census(self.h, kind, C.byref(v)))  # (no arrays: the queue's length)
        q = int(v.queued)
        eq, er = np.zeros(max(1, q), dtype=np.uint32), np.zeros(max(1, q), dtype=np.uint32)
        ar, bf = np.zeros(max(1, q), dtype=np.int32), np.zeros(max(1, q), dtype=np.int32)
        v.entry_query, v.entry_reason = eq.ctypes.data_as(C.POINTER(C.c_uint32)), er.ctypes.data_as(C.POINTER(C.c_uint32))
        v.count_after_rest, v.count_before_fit = ar.ctypes.data_as(C.POINTER(C.c_int32)), bf.ctypes.data_as(C.POINTER(C.c_int32))
        v.entries_cap = q
        nl = int(v.late)
        lq = np.zeros(max(1, nl), dtype=np.uint32)
        v.late_query, v.late_cap = lq.ctypes.data_as(C.POINTER(C.c_uint32)), nl
        self._check(self.lib.loamx_ctx_last_assoc_census(self.h, kind, C.byref(v)))
        return AssocCensus(*[getattr(v, n) for n in ASSOC_CENSUS_SCALARS], np.array(list(v.origin)), eq[:q].copy(), er[:q].copy(),
                           ar[:q].copy(), bf[:q].copy(), lq[:nl].copy())

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    # ---- host entry points -------------------------------------------------------------------------
    def compute_curvature(self, xyz, lidar, fe=None):
        fe = fe or FeatureExtractionParams()
        xyz = _scan(xyz)
        out = np.empty(len(xyz))
        fn = self.lib.loamx_compute_curvature_f32 if xyz.dtype == np.float32 else self.lib.loamx_compute_curvature
        self._check(fn(self.h, _xyzp(xyz), len(xyz), C.byref(lidar), C.byref(fe), _dp(out)))
        return out

    def compute_valid_points(self, xyz, lidar, fe=None):
        fe = fe or FeatureExtractionParams()
        xyz = _scan(xyz)
        out = np.empty(len(xyz), dtype=np.uint8)
        fn = self.lib.loamx_compute_valid_points_f32 if xyz.dtype == np.float32 else self.lib.loamx_compute_valid_points
        self._check(fn(self.h, _xyzp(xyz), len(xyz), C.byref(lidar), C.byref(fe), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out.astype(bool)

    def extract_features(self, xyz, lidar, fe=None):
        """Returns (edge_idx, planar_idx) in the reference's output order. A float32 array takes the FP32-input path."""
        fe = fe or FeatureExtractionParams()
        xyz = _scan(xyz)
        ecap = max(1, self.lib.loamx_edge_capacity(C.byref(lidar), C.byref(fe)))
        pcap = max(1, self.lib.loamx_planar_capacity(C.byref(lidar), C.byref(fe)))
        e = np.empty(ecap, dtype=np.uint32)
        p = np.empty(pcap, dtype=np.uint32)
        ne, npl = C.c_size_t(0), C.c_size_t(0)
        u32p = C.POINTER(C.c_uint32)
        fn = self.lib.loamx_extract_features_f32 if xyz.dtype == np.float32 else self.lib.loamx_extract_features
        self._check(fn(self.h, _xyzp(xyz), len(xyz), C.byref(lidar), C.byref(fe), e.ctypes.data_as(u32p), ecap, C.byref(ne),
                       p.ctypes.data_as(u32p), pcap, C.byref(npl)))
        return e[:ne.value].copy(), p[:npl.value].copy()

    def register_features(self, src_edge, src_planar, tgt_edge, tgt_planar, init_pose=None, reg=None,
                          want_detail=False):
        """Returns (pose7, termination, iterations[, detail dict])."""
        reg = reg or RegistrationParams()
        arrs = [_pts(a) for a in (src_edge, src_planar, tgt_edge, tgt_planar)]
        init = np.ascontiguousarray([0, 0, 0, 1, 0, 0, 0] if init_pose is None else init_pose, dtype=np.float64)
        res = RegResult()
        detail = None
        if want_detail:
            mi = max(1, reg.max_iterations)
            info = (IterInfo * mi)()
            ce, cp = max(1, len(arrs[0])), max(1, len(arrs[1]))
            ep = np.zeros((mi, ce, 2), dtype=np.uint32)
            pp = np.zeros((mi, cp, 2), dtype=np.uint32)
            nep = np.zeros(mi, dtype=np.uint32)
            npp = np.zeros(mi, dtype=np.uint32)
            u32p = C.POINTER(C.c_uint32)
            detail = RegDetail(info, 0, ep.ctypes.data_as(u32p), ce, nep.ctypes.data_as(u32p),
                               pp.ctypes.data_as(u32p), cp, npp.ctypes.data_as(u32p))
        self._check(self.lib.loamx_register_features(
            self.h, _dp(arrs[0]), len(arrs[0]), _dp(arrs[1]), len(arrs[1]), _dp(arrs[2]), len(arrs[2]),
            _dp(arrs[3]), len(arrs[3]), _dp(init), C.byref(reg), C.byref(res),
            C.byref(detail) if detail is not None else None))
        pose = np.array(list(res.pose))
        if want_detail:
            d = dict(iterations=[dict(target_T_source_init=np.array(list(info[i].target_T_source_init)),
                                      estimate_update=np.array(list(info[i].estimate_update)),
                                      n_edge=info[i].n_edge_associations, n_plane=info[i].n_plane_associations,
                                      edge_pairs=ep[i, :nep[i]].copy(), plane_pairs=pp[i, :npp[i]].copy())
                                 for i in range(detail.n_iter_info)])
            return pose, res.termination, res.iterations, d
        return pose, res.termination, res.iterations

    # ---- rows a16-a19 one by one (geometry_internal / kdtree_internal / registration_internal of the reference) ----
    def fit_lines(self, points):
        """geometry_internal::fitLine over (n_sets, k, 3) points -> (a (n,3), b (n,3), cond (n,))"""
        pts = np.ascontiguousarray(points, dtype=np.float64)
        n, k = pts.shape[0], pts.shape[1]
        out, cond = np.zeros((n, 6)), np.zeros(n)
        self._check(self.lib.loamx_fit_lines(self.h, _dp(pts), n, k, _dp(out), _dp(cond)))
        return out[:, :3].copy(), out[:, 3:].copy(), cond

    def fit_planes(self, points):
        """geometry_internal::fitPlane over (n_sets, k, 3) points -> (normal (n,3), d (n,), avg signed distance (n,))"""
        pts = np.ascontiguousarray(points, dtype=np.float64)
        n, k = pts.shape[0], pts.shape[1]
        out, avg = np.zeros((n, 4)), np.zeros(n)
        self._check(self.lib.loamx_fit_planes(self.h, _dp(pts), n, k, _dp(out), _dp(avg)))
        return out[:, :3].copy(), out[:, 3].copy(), avg

    def knn_search(self, index, which_set, queries, k, max_dist=-1.0):
        """kdtree_internal::knnSearch for every query against one set of a target index -> list of index arrays"""
        q = _pts(queries)
        idx, cnt = np.zeros((len(q), max(k, 1)), dtype=np.uint32), np.zeros(len(q), dtype=np.uint32)
        self._check(self.lib.loamx_knn_search(self.h, index, which_set, _dp(q), len(q), k, float(max_dist), idx.ctypes.data, cnt.ctypes.data))
        return [idx[i, :cnt[i]].copy() for i in range(len(q))]

    def associate(self, src_edge, src_planar, tgt_edge, tgt_planar, pose=None, reg=None):
        """One association pass of the registration kernels at `pose` (registration.cpp:23-103), per source feature:
        dict(edge=..., plane=...) of dict(nn (list of index arrays), valid, moved, prim)."""
        reg = reg or RegistrationParams()
        arrs = [_pts(a) for a in (src_edge, src_planar, tgt_edge, tgt_planar)]
        pose = np.ascontiguousarray([0, 0, 0, 1, 0, 0, 0] if pose is None else pose, dtype=np.float64)
        n, k, pw = [len(arrs[0]), len(arrs[1])], [int(reg.num_edge_neighbors), int(reg.num_plane_neighbors)], [6, 4]
        bufs = []
        for kind in range(2):
            bufs.append(dict(cnt=np.zeros(n[kind], dtype=np.uint32), idx=np.full((n[kind], max(k[kind], 1)), 0xFFFFFFFF, dtype=np.uint32),
                             valid=np.zeros(n[kind], dtype=np.uint8), moved=np.zeros((n[kind], 3)), prim=np.zeros((n[kind], pw[kind]))))
        queues = np.zeros(4, dtype=np.uint32)
        d = AssocDump(*([b[f].ctypes.data for b in bufs for f in ("cnt", "idx", "valid", "moved", "prim")] + [queues.ctypes.data]))
        self._check(self.lib.loamx_associate(self.h, _dp(arrs[0]), n[0], _dp(arrs[1]), n[1], _dp(arrs[2]), len(arrs[2]), _dp(arrs[3]),
                                             len(arrs[3]), _dp(pose), C.byref(reg), C.byref(d)))
        out = {}
        for kind, name in enumerate(("edge", "plane")):
            b = bufs[kind]
            out[name] = dict(nn=[b["idx"][i, :b["cnt"][i]].copy() for i in range(n[kind])], valid=b["valid"].astype(bool),
                             moved=b["moved"], prim=b["prim"], queued=(int(queues[kind]), int(queues[2 + kind])))
        return out

    # ---- persistent target index (scan-to-map) -----------------------------------------------------------
    def target_index(self, tgt_edge, tgt_planar, reg=None):
        reg = reg or RegistrationParams()
        te, tp = _pts(tgt_edge), _pts(tgt_planar)
        h = C.c_void_p()
        self._check(self.lib.loamx_target_index_create(self.h, _dp(te), len(te), _dp(tp), len(tp), C.byref(reg), C.byref(h)))
        return h

    def target_index_insert(self, index, edge, planar):
        """Appends points to a target index (same result as an index built over the concatenated sets)."""
        e, p = _pts(edge), _pts(planar)
        self._check(self.lib.loamx_target_index_insert(self.h, index, _dp(e), len(e), _dp(p), len(p)))

    def target_index_size(self, index):
        ne, npl = C.c_size_t(0), C.c_size_t(0)
        self._check(self.lib.loamx_target_index_size(index, C.byref(ne), C.byref(npl)))
        return ne.value, npl.value

    def target_index_stats(self, index):
        """(full builds of a feature kind's grid, merges into an existing grid) so far"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.loamx_target_index_stats(index, C.byref(a), C.byref(b)))
        return a.value, b.value

    def target_index_census(self, index, which_set, arrays=True):
        """One kind of a persistent index as it lies on the device and the build form behind it (include/loamx.h:
        loamx_target_index_census), as an IndexCensus. arrays: cell_start (nx ny nz + 1; None while table_valid == 0), the
        cell-sorted points xyz (n, 3) with orig (n,), and rel (3, n + 4) with the pad entries; False: None for all four."""
        v = IndexCensusStruct()
        self._check(self.lib.loamx_target_index_census(self.h, index, which_set, C.byref(v)))
        cs = xyz = orig = rel = None
        if arrays:
            n, ncell = int(v.n), int(v.nx) * int(v.ny) * int(v.nz)
            cs, xyz = np.zeros(ncell + 1, dtype=np.uint32), np.zeros((n, 3))
            orig, rel = np.zeros(n, dtype=np.uint32), np.zeros((3, n + 4), dtype=np.float32)
            v.cell_start, v.cell_start_cap = cs.ctypes.data_as(C.POINTER(C.c_uint32)), ncell + 1
            v.xyz, v.orig, v.points_cap = _dp(xyz), orig.ctypes.data_as(C.POINTER(C.c_uint32)), n
            v.rel, v.rel_cap = rel.ctypes.data_as(C.POINTER(C.c_float)), n + 4
            self._check(self.lib.loamx_target_index_census(self.h, index, which_set, C.byref(v)))
            if not v.table_valid:
                cs = None
        return IndexCensus(int(v.n), int(v.capacity), np.array(list(v.origin)), v.h, v.inv_h, (v.nx, v.ny, v.nz), v.n_points, v.build,
                           v.table_valid, int(v.table_entries), v.lds_passes, v.scan_tiles, v.last_op, int(v.full_builds), int(v.merges),
                           cs, xyz, orig, rel)

    # ---- map upkeep: voxel-filtered insert, crop, read-back (include/loamx.h, "map upkeep") ----------------
    @staticmethod
    def _pose_arg(pose):
        """None (identity) or a contiguous pose7 -> what the C ABI takes (keep the array alive during the call)"""
        if pose is None:
            return None, None
        p = np.ascontiguousarray(pose, dtype=np.float64)
        if p.size != 7:
            raise ValueError("a pose has 7 values: qx, qy, qz, qw, tx, ty, tz")
        return p, _dp(p)

    def target_index_points(self, index, which_set, first=0, count=None):
        """the points of one set (0 edge, 1 planar) in index order, as an (n, 3) array"""
        if count is None:
            count = self.target_index_size(index)[which_set] - first
        out = np.empty((max(int(count), 0), 3))
        self._check(self.lib.loamx_target_index_points(self.h, index, which_set, first, count, _dp(out)))
        return out

    def voxel_filter_dev(self, d_xyz, n, leaf, d_xyz_out, d_n_out, d_src_idx=0, pose=None):
        """transform + voxel filter of n device points (loamx_voxel_filter_dev); asynchronous on the context's stream"""
        keep, p = self._pose_arg(pose)
        self._check(self.lib.loamx_voxel_filter_dev(self.h, d_xyz or None, n, p, float(leaf), d_xyz_out or None, d_src_idx or None, d_n_out))

    def voxel_filter(self, points, leaf, pose=None):
        """Host convenience: uploads the points, runs voxel_filter_dev and returns (kept points (m, 3), src_idx (m,))."""
        pts = _pts(points)
        n = len(pts)
        d_in, d_out, d_idx, d_n = self.alloc(max(pts.nbytes, 8)), self.alloc(max(pts.nbytes, 8)), self.alloc(max(4 * n, 8)), self.alloc(8)
        try:
            if n:
                d_in.upload(pts)
            self.voxel_filter_dev(d_in.ptr, n, leaf, d_out.ptr, d_n.ptr, d_idx.ptr, pose)
            self.synchronize()
            m = int(d_n.download(np.uint32, 1)[0])
            if m == 0:
                return np.empty((0, 3)), np.empty(0, dtype=np.uint32)
            return d_out.download(np.float64, 3 * m).reshape(-1, 3), d_idx.download(np.uint32, m)
        finally:
            for b in (d_in, d_out, d_idx, d_n):
                b.free()

    def target_index_insert_filtered(self, index, edge, planar, pose=None, edge_leaf=0.2, planar_leaf=0.4):
        """Adds pose.act(point) for every point whose voxel (edge_leaf / planar_leaf; <= 0: unfiltered) holds neither a
        point of the map nor an earlier point of this call. Returns (n_edge_added, n_planar_added)."""
        e, p = _pts(edge), _pts(planar)
        keep, pp = self._pose_arg(pose)
        ne, npl = C.c_size_t(0), C.c_size_t(0)
        self._check(self.lib.loamx_target_index_insert_filtered(self.h, index, _dp(e), len(e), _dp(p), len(p), pp, float(edge_leaf),
                                                                float(planar_leaf), C.byref(ne), C.byref(npl)))
        return ne.value, npl.value

    def target_index_crop(self, index, lo, hi):
        """Keeps the points inside the box [lo, hi] (inclusive). Returns (edge points removed, planar points removed)."""
        lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
        if lo.size != 3 or hi.size != 3:
            raise ValueError("target_index_crop: lo and hi have 3 values each")
        ne, npl = C.c_size_t(0), C.c_size_t(0)
        self._check(self.lib.loamx_target_index_crop(self.h, index, _dp(lo), _dp(hi), C.byref(ne), C.byref(npl)))
        return ne.value, npl.value

    def target_index_destroy(self, index):
        self.lib.loamx_target_index_destroy(self.h, index)

    def register_features_indexed(self, index, src_edge, src_planar, init_pose=None, reg=None):
        reg = reg or RegistrationParams()
        se, sp = _pts(src_edge), _pts(src_planar)
        init = np.ascontiguousarray([0, 0, 0, 1, 0, 0, 0] if init_pose is None else init_pose, dtype=np.float64)
        res = RegResult()
        self._check(self.lib.loamx_register_features_indexed(self.h, index, _dp(se), len(se), _dp(sp), len(sp), _dp(init),
                                                             C.byref(reg), C.byref(res), None))
        return np.array(list(res.pose)), res.termination, res.iterations

    # ---- registration information matrix (include/loamx.h: loamx_reg_information) -----------------------
    def registration_information(self, src_edge, src_planar, tgt_edge, tgt_planar, pose=None, reg=None):
        """The information matrix of the pair's residuals at `pose` (target_T_source; None = identity), as a RegInformation."""
        reg = reg or RegistrationParams()
        arrs = [_pts(a) for a in (src_edge, src_planar, tgt_edge, tgt_planar)]
        pose = np.ascontiguousarray([0, 0, 0, 1, 0, 0, 0] if pose is None else pose, dtype=np.float64)
        if pose.size != 7:
            raise ValueError("a pose has 7 values: qx, qy, qz, qw, tx, ty, tz")
        info = RegInformation()
        self._check(self.lib.loamx_registration_information(self.h, _dp(arrs[0]), len(arrs[0]), _dp(arrs[1]), len(arrs[1]), _dp(arrs[2]),
                                                            len(arrs[2]), _dp(arrs[3]), len(arrs[3]), _dp(pose), C.byref(reg), C.byref(info)))
        return info

    def registration_information_indexed(self, index, src_edge, src_planar, pose=None, reg=None):
        """the same against a persistent target index (scan-to-map)"""
        reg = reg or RegistrationParams()
        se, sp = _pts(src_edge), _pts(src_planar)
        pose = np.ascontiguousarray([0, 0, 0, 1, 0, 0, 0] if pose is None else pose, dtype=np.float64)
        if pose.size != 7:
            raise ValueError("a pose has 7 values: qx, qy, qz, qw, tx, ty, tz")
        info = RegInformation()
        self._check(self.lib.loamx_registration_information_indexed(self.h, index, _dp(se), len(se), _dp(sp), len(sp), _dp(pose),
                                                                    C.byref(reg), C.byref(info)))
        return info

    def registration_information_batch_dev(self, n_pairs, d_src_edge, d_n_src_edge, d_src_planar, d_n_src_planar, d_tgt_edge,
                                           d_n_tgt_edge, d_tgt_planar, d_n_tgt_planar, edge_stride, planar_stride, d_pose, reg, d_info):
        """n_pairs device-resident pairs (layout of register_features_batch_dev) at the poses d_pose (n_pairs x 7 device doubles,
        0 = identity) -> n_pairs device records (INFORMATION_DTYPE). Asynchronous on the context's stream."""
        self._check(self.lib.loamx_registration_information_batch_dev(
            self.h, n_pairs, d_src_edge, d_n_src_edge, d_src_planar, d_n_src_planar, d_tgt_edge, d_n_tgt_edge, d_tgt_planar,
            d_n_tgt_planar, edge_stride, planar_stride, d_pose or None, C.byref(reg), d_info))

    # ---- device-resident batch entry points (raw device pointers as ints) -----------------------------
    def edge_capacity(self, lidar, fe):
        return self.lib.loamx_edge_capacity(C.byref(lidar), C.byref(fe))

    def planar_capacity(self, lidar, fe):
        return self.lib.loamx_planar_capacity(C.byref(lidar), C.byref(fe))

    def extract_features_batch_dev(self, d_xyz, n_scans, lidar, fe, d_edge_idx, d_n_edge, d_edge_xyz, d_planar_idx,
                                   d_n_planar, d_planar_xyz, f32=False):
        fn = self.lib.loamx_extract_features_batch_dev_f32 if f32 else self.lib.loamx_extract_features_batch_dev
        self._check(fn(self.h, d_xyz, n_scans, C.byref(lidar), C.byref(fe), d_edge_idx, d_n_edge, d_edge_xyz, d_planar_idx,
                       d_n_planar, d_planar_xyz))

    def register_features_batch_dev(self, n_pairs, d_src_edge, d_n_src_edge, d_src_planar, d_n_src_planar,
                                    d_tgt_edge, d_n_tgt_edge, d_tgt_planar, d_n_tgt_planar, edge_stride,
                                    planar_stride, d_init, reg, d_results):
        self._check(self.lib.loamx_register_features_batch_dev(
            self.h, n_pairs, d_src_edge, d_n_src_edge, d_src_planar, d_n_src_planar, d_tgt_edge, d_n_tgt_edge,
            d_tgt_planar, d_n_tgt_planar, edge_stride, planar_stride, d_init, C.byref(reg), d_results))

    def register_scan_pairs_dev(self, d_xyz, n_pairs, lidar, fe, reg, d_results, f32=False, d_info=None):
        """d_info: device room for n_pairs information records (INFORMATION_DTYPE), taken at the result poses (the "_info" form)"""
        if d_info:
            fn = self.lib.loamx_register_scan_pairs_info_dev_f32 if f32 else self.lib.loamx_register_scan_pairs_info_dev
            self._check(fn(self.h, d_xyz, n_pairs, C.byref(lidar), C.byref(fe), C.byref(reg), d_results, d_info))
            return
        fn = self.lib.loamx_register_scan_pairs_dev_f32 if f32 else self.lib.loamx_register_scan_pairs_dev
        self._check(fn(self.h, d_xyz, n_pairs, C.byref(lidar), C.byref(fe), C.byref(reg), d_results))

    def register_scan_pairs(self, xyz, n_pairs, lidar, fe=None, reg=None, out=None):
        """Host memory in, host memory out (loamx_register_scan_pairs): xyz = a C-contiguous float64 / float32 array (or an
        integer address + dtype via `xyz=(ptr, np.float32)`) of n_pairs x 2 scans, target scan first; returns the result
        records (RESULT_DTYPE). Pinned memory (e.g. a torch pin_memory tensor's numpy view) lets the uploads overlap.
        The address form states the buffer's element count: `xyz=(ptr, np.float32, count)`. Arguments that do not hold
        n_pairs x 2 x H x W points, or an `out` that is not n_pairs RESULT_DTYPE records, raise ValueError before anything
        is copied."""
        fe, reg = fe or FeatureExtractionParams(), reg or RegistrationParams()
        if isinstance(xyz, tuple):
            if len(xyz) != 3:
                raise ValueError("register_scan_pairs: the address form is xyz=(ptr, dtype, element count)")
            ptr, dt, size = xyz
            dt = np.dtype(dt)
        else:
            if not isinstance(xyz, np.ndarray) or not xyz.flags["C_CONTIGUOUS"]:
                raise ValueError("register_scan_pairs: xyz must be a C-contiguous numpy array")
            ptr, dt, size = xyz.ctypes.data, xyz.dtype, xyz.size
        if dt not in (np.float64, np.float32):
            raise ValueError(f"register_scan_pairs: xyz must be float64 or float32, not {dt}")
        f32 = dt == np.float32
        need = int(n_pairs) * 2 * int(lidar.scan_lines) * int(lidar.points_per_line) * 3
        if int(size) < need:
            raise ValueError(f"register_scan_pairs: xyz holds {int(size)} values, {n_pairs} pairs need {need}")
        if out is not None and (not isinstance(out, np.ndarray) or out.dtype != RESULT_DTYPE or not out.flags["C_CONTIGUOUS"]
                                or out.size < n_pairs):
            raise ValueError(f"register_scan_pairs: out must be a C-contiguous array of at least {n_pairs} RESULT_DTYPE records")
        res = out if out is not None else np.zeros(n_pairs, dtype=RESULT_DTYPE)
        fn = self.lib.loamx_register_scan_pairs_f32 if f32 else self.lib.loamx_register_scan_pairs
        self._check(fn(self.h, ptr, n_pairs, C.byref(lidar), C.byref(fe), C.byref(reg), res.ctypes.data))
        return res

    # ---- scan sequences: scan i is the source of pair i - 1 and the target of pair i ------------------------
    def register_scan_sequence_dev(self, d_xyz, n_scans, lidar, fe, reg, d_results, d_init=0, f32=False, d_info=None):
        """n_scans device-resident scans back to back -> n_scans - 1 device records (pair p: scan p target, scan p + 1
        source); d_init: (n_scans - 1) x 7 device doubles or 0 (identity). Asynchronous on the context's stream.
        d_info: device room for n_scans - 1 information records, taken at the result poses (the "_info" form)."""
        if d_info:
            fn = self.lib.loamx_register_scan_sequence_info_dev_f32 if f32 else self.lib.loamx_register_scan_sequence_info_dev
            self._check(fn(self.h, d_xyz, n_scans, C.byref(lidar), C.byref(fe), C.byref(reg), d_init or None, d_results, d_info))
            return
        fn = self.lib.loamx_register_scan_sequence_dev_f32 if f32 else self.lib.loamx_register_scan_sequence_dev
        self._check(fn(self.h, d_xyz, n_scans, C.byref(lidar), C.byref(fe), C.byref(reg), d_init or None, d_results))

    def register_scan_sequence(self, xyz, n_scans, lidar, fe=None, reg=None, init=None, out=None):
        """Host memory in, host memory out (loamx_register_scan_sequence): xyz = a C-contiguous float64 / float32 array
        (or `xyz=(ptr, dtype, element count)`) of n_scans consecutive scans; returns the n_scans - 1 result records
        (RESULT_DTYPE). init: None or a C-contiguous float64 array of (n_scans - 1) x 7 initial poses. Arguments that do
        not hold n_scans x H x W points, or an `out` / `init` of the wrong type or size, raise ValueError before anything
        is copied."""
        fe, reg = fe or FeatureExtractionParams(), reg or RegistrationParams()
        n_scans = int(n_scans)
        if n_scans < 0:
            raise ValueError("register_scan_sequence: n_scans must not be negative")
        n_pairs = max(n_scans - 1, 0)
        if isinstance(xyz, tuple):
            if len(xyz) != 3:
                raise ValueError("register_scan_sequence: the address form is xyz=(ptr, dtype, element count)")
            ptr, dt, size = xyz
            dt = np.dtype(dt)
        else:
            if not isinstance(xyz, np.ndarray) or not xyz.flags["C_CONTIGUOUS"]:
                raise ValueError("register_scan_sequence: xyz must be a C-contiguous numpy array")
            ptr, dt, size = xyz.ctypes.data, xyz.dtype, xyz.size
        if dt not in (np.float64, np.float32):
            raise ValueError(f"register_scan_sequence: xyz must be float64 or float32, not {dt}")
        f32 = dt == np.float32
        need = n_scans * int(lidar.scan_lines) * int(lidar.points_per_line) * 3
        if int(size) < need:
            raise ValueError(f"register_scan_sequence: xyz holds {int(size)} values, {n_scans} scans need {need}")
        if out is not None and (not isinstance(out, np.ndarray) or out.dtype != RESULT_DTYPE or not out.flags["C_CONTIGUOUS"]
                                or out.size < n_pairs):
            raise ValueError(f"register_scan_sequence: out must be a C-contiguous array of at least {n_pairs} RESULT_DTYPE records")
        if init is not None and (not isinstance(init, np.ndarray) or init.dtype != np.float64 or not init.flags["C_CONTIGUOUS"]
                                 or init.size < n_pairs * 7):
            raise ValueError(f"register_scan_sequence: init must be a C-contiguous float64 array of at least {n_pairs} x 7 values")
        res = out if out is not None else np.zeros(n_pairs, dtype=RESULT_DTYPE)
        fn = self.lib.loamx_register_scan_sequence_f32 if f32 else self.lib.loamx_register_scan_sequence
        self._check(fn(self.h, ptr, n_scans, C.byref(lidar), C.byref(fe), C.byref(reg),
                       init.ctypes.data if init is not None and n_pairs else None, res.ctypes.data))
        return res

    def compose_trajectory_dev(self, d_results, n_pairs, d_world_T_scan, origin=None):
        """d_world_T_scan[(n_pairs + 1) x 7] <- origin, origin (+) pose 0, ... (loamx_compose_trajectory_dev); origin: a
        host pose7 or None (identity). Asynchronous on the context's stream."""
        o = None if origin is None else np.ascontiguousarray(origin, dtype=np.float64)
        if o is not None and o.size != 7:
            raise ValueError("compose_trajectory_dev: origin must be a pose of 7 values")
        self._check(self.lib.loamx_compose_trajectory_dev(self.h, d_results, n_pairs, _dp(o) if o is not None else None, d_world_T_scan))

    def deskew_scans_dev(self, d_xyz, n_scans, lidar, d_motion, d_xyz_out, ref_fraction=1.0, f32=False):
        """motion correction of n_scans device-resident scans (loamx_deskew_scans_dev); d_xyz_out may equal d_xyz"""
        fn = self.lib.loamx_deskew_scans_dev_f32 if f32 else self.lib.loamx_deskew_scans_dev
        self._check(fn(self.h, d_xyz, n_scans, C.byref(lidar), d_motion, float(ref_fraction), d_xyz_out))

    def deskew_scans(self, xyz, lidar, motions, ref_fraction=1.0):
        """Uploads the scans (float64 or float32, any shape that holds whole scans) and one motion (pose7) per scan,
        runs loamx_deskew_scans_dev and returns the corrected scans in the shape and dtype of `xyz`."""
        a = np.asarray(xyz)
        if a.dtype != np.float32:
            a = np.asarray(a, dtype=np.float64)
        a = np.ascontiguousarray(a)
        per_scan = int(lidar.scan_lines) * int(lidar.points_per_line) * 3
        if per_scan == 0 or a.size % per_scan:
            raise ValueError("deskew_scans: xyz does not hold whole scans")
        n_scans = a.size // per_scan
        m = np.ascontiguousarray(motions, dtype=np.float64)
        if m.size != n_scans * 7:
            raise ValueError(f"deskew_scans: {n_scans} scans need {n_scans} motions of 7 values")
        if n_scans == 0:
            return a.copy()
        d_xyz, d_m = self.alloc(a.nbytes), self.alloc(m.nbytes)
        try:
            d_xyz.upload(a), d_m.upload(m)
            self.deskew_scans_dev(d_xyz.ptr, n_scans, lidar, d_m.ptr, d_xyz.ptr, ref_fraction, f32=a.dtype == np.float32)
            self.synchronize()
            return d_xyz.download(a.dtype, a.size).reshape(a.shape)
        finally:
            d_xyz.free(), d_m.free()

    # ---- unordered clouds into scans (include/loamx.h, "unordered clouds into scans") ----------------------
    def scan_layout(self, lidar, params=None):
        return ScanLayout(self, lidar, params)

    def organize_clouds_dev(self, layout, d_points, point_stride, cloud_offsets, d_scans, d_rings=0, d_src_idx=0, d_stats=0, f32=False):
        """len(cloud_offsets) - 1 device-resident clouds back to back -> as many scans (loamx_organize_clouds_dev[_f32]).
        cloud_offsets: host integers, ascending point offsets; d_rings / d_src_idx / d_stats: device addresses or 0.
        Asynchronous on the context's stream."""
        off = np.ascontiguousarray(cloud_offsets)
        if off.ndim != 1 or off.size < 1 or off.dtype.kind not in "iu":
            raise ValueError("organize_clouds_dev: cloud_offsets is a 1-d integer array of n_clouds + 1 offsets")
        if off.dtype.kind == "i" and (off < 0).any():
            raise ValueError("organize_clouds_dev: negative offset")
        off = off.astype(np.uint64)
        fn = self.lib.loamx_organize_clouds_dev_f32 if f32 else self.lib.loamx_organize_clouds_dev
        self._check(fn(self.h, layout._handle(), d_points or None, int(point_stride), d_rings or None,
                       off.ctypes.data_as(C.POINTER(C.c_size_t)), off.size - 1, d_scans or None, d_src_idx or None, d_stats or None))

    def organize_cloud(self, points, layout, rings=None):
        """One unordered cloud in host memory, (n, 3) or (n, 4) float64 / float32 -> (scan (H W, 3) in the cloud's dtype,
        src_idx (H W,) uint32 with NO_POINT for an empty cell, stats = uint32 [filled, invalid, outside, collisions])."""
        pts = np.asarray(points)
        if pts.dtype != np.float32:
            pts = np.asarray(pts, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] < 3:
            raise ValueError(f"organize_cloud: points must be (n, 3) or (n, k >= 3), not {pts.shape}")
        pts = np.ascontiguousarray(pts)
        n, stride = pts.shape
        r = None
        if rings is not None:
            r = np.asarray(rings)
            if r.dtype != np.uint16:
                if r.dtype.kind not in "iu" or (r.size and (r.min() < 0 or r.max() > 0xFFFF)):
                    raise ValueError("organize_cloud: rings must be integers in 0 .. 65535")
                r = r.astype(np.uint16)
            r = np.ascontiguousarray(r).reshape(-1)
            if r.size != n:
                raise ValueError(f"organize_cloud: {r.size} ring numbers for {n} points")
        scan = np.empty((layout.cells, 3), dtype=pts.dtype)
        src, stats = np.empty(layout.cells, dtype=np.uint32), np.empty(4, dtype=np.uint32)
        fn = self.lib.loamx_organize_cloud_f32 if pts.dtype == np.float32 else self.lib.loamx_organize_cloud
        self._check(fn(self.h, layout._handle(), pts.ctypes.data, stride, r.ctypes.data if r is not None else None, n, scan.ctypes.data,
                       src.ctypes.data, stats.ctypes.data))
        return scan, src, stats

    # ---- scan segmentation (include/loamx.h, "scan segmentation") ----------------------------------------------
    def segment_scans_dev(self, d_scans, n_scans, lidar, params=None, d_classes=0, d_labels=0, d_sizes=0, d_filtered=0, d_clusters=0,
                          max_clusters=0, d_stats=0, f32=False):
        """n_scans device-resident scans -> classes, labels, sizes, the filtered scans, the cluster tables (max_clusters records
        per scan) and the stats (loamx_segment_scans_dev[_f32]); every output is a device address or 0. d_filtered may equal
        d_scans. Asynchronous on the context's stream."""
        if int(n_scans) < 0 or int(max_clusters) < 0:
            raise ValueError("segment_scans_dev: n_scans and max_clusters must be >= 0")
        st = (params or SegmentParams()).struct()
        fn = self.lib.loamx_segment_scans_dev_f32 if f32 else self.lib.loamx_segment_scans_dev
        self._check(fn(self.h, d_scans or None, int(n_scans), C.byref(lidar), C.byref(st), d_classes or None, d_labels or None, d_sizes or None,
                       d_filtered or None, d_clusters or None, int(max_clusters), d_stats or None))

    def segment_scan(self, scan, lidar, params=None):
        """One organised scan in host memory, float64 or float32 -> (classes (H W,) uint8, labels (H W,) uint32 with
        SEGMENT_NO_LABEL outside the components, sizes (H W,) uint32, filtered (H W, 3) in the scan's dtype, clusters = the accepted
        components as SEGMENT_CLUSTER_DTYPE records in ascending root order, stats = uint32[8], see SEGMENT_STATS)."""
        a = np.asarray(scan)
        if a.dtype != np.float32:
            a = np.asarray(a, dtype=np.float64)
        cells = int(lidar.scan_lines) * int(lidar.points_per_line)
        if a.size != cells * 3:
            raise ValueError(f"segment_scan: the scan holds {a.size} scalars, the lidar parameters ask for {cells} x 3")
        a = np.ascontiguousarray(a.reshape(-1, 3))
        st = (params or SegmentParams()).struct()
        classes, labels, sizes = np.empty(cells, np.uint8), np.empty(cells, np.uint32), np.empty(cells, np.uint32)
        filtered, clusters, stats = np.empty_like(a), np.empty(cells, SEGMENT_CLUSTER_DTYPE), np.zeros(8, np.uint32)
        fn = self.lib.loamx_segment_scan_f32 if a.dtype == np.float32 else self.lib.loamx_segment_scan
        self._check(fn(self.h, a.ctypes.data, C.byref(lidar), C.byref(st), classes.ctypes.data, labels.ctypes.data, sizes.ctypes.data,
                       filtered.ctypes.data, clusters.ctypes.data, cells, stats.ctypes.data))
        return classes, labels, sizes, filtered, clusters[:int(stats[7])].copy(), stats

    def last_raycast_census(self):
        """one RAYCAST_CENSUS_DTYPE record of the context's last cast_rays / render_scans call: rays, tested visits, look-ups made
        and the rays by status (loamx_ctx_last_raycast_census; synchronises)"""
        c = np.zeros(1, dtype=RAYCAST_CENSUS_DTYPE)
        self._check(self.lib.loamx_ctx_last_raycast_census(self.h, c.ctypes.data))
        return c[0]

    def last_segment_census(self):
        """The last segmentation call of this context (loamx_ctx_last_segment_census): tile shape, tiles per scan, the connected
        edges that went through the global union, and whether the tile form ran."""
        v = (C.c_uint64 * 5)()
        self._check(self.lib.loamx_ctx_last_segment_census(self.h, v))
        return SegmentCensus(int(v[0]), int(v[1]), int(v[2]), int(v[3]), bool(v[4]))

    # ---- map cleaning (include/loamx.h, "map cleaning") ---------------------------------------------------------
    def visibility_votes_dev(self, layout, d_points, point_stride, n_points, d_scans, n_scans, d_poses, d_votes, params=None, accumulate=False,
                             f32=False):
        """The votes of n_points device-resident map points (double, world frame) over n_scans device-resident scans of the
        layout's shape at d_poses (device, n_scans x 7) into d_votes (n_points VISIBILITY_VOTES_DTYPE records), written or, with
        accumulate, added to (loamx_visibility_votes_dev[_f32]; f32 is the scans' type). Asynchronous on the context's stream."""
        if int(n_points) < 0 or int(n_scans) < 0:
            raise ValueError("visibility_votes_dev: n_points and n_scans must be >= 0")
        st = (params or VisibilityParams()).struct()
        fn = self.lib.loamx_visibility_votes_dev_f32 if f32 else self.lib.loamx_visibility_votes_dev
        self._check(fn(self.h, layout._handle(), d_points or None, int(point_stride), int(n_points), d_scans or None, int(n_scans), d_poses or None,
                       C.byref(st), 1 if accumulate else 0, d_votes or None))

    def visibility_votes(self, points, scans, poses, layout, params=None):
        """Host form: points (n, k >= 3) float64 world, scans (n_scans, H W, 3) float64 or float32, poses (n_scans, 7) -> (n,)
        VISIBILITY_VOTES_DTYPE (loamx_visibility_votes[_f32]; synchronous)."""
        pts = np.ascontiguousarray(points, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] < 3:
            raise ValueError(f"visibility_votes: points must be (n, k >= 3), not {pts.shape}")
        sc = np.asarray(scans)
        if sc.dtype != np.float32:
            sc = np.asarray(sc, dtype=np.float64)
        sc = np.ascontiguousarray(sc)
        if sc.size % (layout.cells * 3):
            raise ValueError(f"visibility_votes: the scans hold {sc.size} scalars, no multiple of {layout.cells} x 3")
        n_scans = sc.size // (layout.cells * 3)
        po = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
        if len(po) != n_scans:
            raise ValueError(f"visibility_votes: {len(po)} poses for {n_scans} scans")
        st = (params or VisibilityParams()).struct()
        votes = np.zeros(len(pts), dtype=VISIBILITY_VOTES_DTYPE)
        fn = self.lib.loamx_visibility_votes_f32 if sc.dtype == np.float32 else self.lib.loamx_visibility_votes
        self._check(fn(self.h, layout._handle(), pts.ctypes.data if len(pts) else None, pts.shape[1], len(pts), sc.ctypes.data if n_scans else None,
                       n_scans, po.ctypes.data if n_scans else None, C.byref(st), votes.ctypes.data if len(pts) else None))
        return votes

    def visibility_filter_dev(self, d_votes, n_points, d_n_static_out, params=None, d_points=0, point_stride=3, d_dynamic_out=0, d_static_xyz_out=0,
                              d_static_index_out=0, capacity=0):
        """The decision per point and the ordered compaction of the points that stay (loamx_visibility_filter_dev); every output
        but d_n_static_out is a device address or 0. Asynchronous on the context's stream."""
        if int(n_points) < 0 or int(capacity) < 0:
            raise ValueError("visibility_filter_dev: n_points and capacity must be >= 0")
        st = (params or VisibilityParams()).struct()
        self._check(self.lib.loamx_visibility_filter_dev(self.h, d_votes or None, int(n_points), C.byref(st), d_points or None, int(point_stride),
                                                         d_dynamic_out or None, d_static_xyz_out or None, d_static_index_out or None, int(capacity),
                                                         d_n_static_out or None))

    def last_visibility_census(self):
        """The last votes call of this context (loamx_ctx_last_visibility_census): the form (1 ranges, 0 scans), the workgroup rows
        the scans were dealt over, the pairs in range and the pairs that had a cell. Synchronises."""
        v = VisibilityCensusStruct()
        self._check(self.lib.loamx_ctx_last_visibility_census(self.h, C.byref(v)))
        return VisibilityCensus(int(v.form), int(v.scan_chunks), int(v.in_range_pairs), int(v.projected_pairs))

    # ---- place recognition (include/loamx.h, "place recognition") --------------------------------------------
    def place_db(self, params=None):
        return PlaceDb(self, params)

    # ---- cloud map (include/loamx.h, "cloud map") ---------------------------------------------------------------
    def cloud_map(self, params=None, max_voxels=1 << 20):
        return CloudMap(self, params, max_voxels)

    def surfel_map(self, params=None, max_voxels=1 << 20):
        return SurfelMap(self, params, max_voxels)

    def occupancy_map(self, params=None, max_voxels=1 << 20):
        return OccupancyMap(self, params, max_voxels)

    @staticmethod
    def _pgo_params(params):
        return (params or PgoParams()).struct()

    def pose_graph_optimize_dev(self, d_poses, n_poses, d_edges, n_edges, d_fixed=0, params=None, d_summary=0):
        """loamx_pose_graph_optimize_dev: d_poses (n_poses x 7) corrected in place on the context's stream; d_fixed: n_poses bytes or 0
        (pose 0 only); d_summary: one PGO_SUMMARY_DTYPE record or 0"""
        ptr = lambda b: b.ptr if isinstance(b, DeviceBuffer) else b
        p = self._pgo_params(params)
        self._check(self.lib.loamx_pose_graph_optimize_dev(self.h, ptr(d_poses), n_poses, ptr(d_fixed) or None, ptr(d_edges), n_edges,
                                                           C.byref(p), ptr(d_summary) or None))

    def pose_graph_optimize(self, poses, edges, fixed=None, params=None):
        """The host form -> (poses (n, 7), summary record of PGO_SUMMARY_DTYPE). edges: PGO_EDGE_DTYPE records."""
        poses = np.array(poses, dtype=np.float64).reshape(-1, 7)
        edges = np.ascontiguousarray(edges, dtype=PGO_EDGE_DTYPE)
        fx = None if fixed is None else np.ascontiguousarray(np.asarray(fixed) != 0, dtype=np.uint8)
        if fx is not None and len(fx) != len(poses):
            raise ValueError("pose_graph_optimize: one fixed flag per pose")
        summary = np.zeros(1, dtype=PGO_SUMMARY_DTYPE)
        p = self._pgo_params(params)
        self._check(self.lib.loamx_pose_graph_optimize(self.h, poses.ctypes.data, len(poses), None if fx is None else fx.ctypes.data,
                                                       edges.ctypes.data if len(edges) else None, len(edges), C.byref(p), summary.ctypes.data))
        return poses, summary[0]

    def pose_graph_linearize(self, poses, edges, huber_delta=0.0):
        """e, chi2, weight, A, B of every edge at the given poses (PGO_LINEARIZATION_DTYPE), by the solver's own kernel"""
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
        edges = np.ascontiguousarray(edges, dtype=PGO_EDGE_DTYPE)
        out = np.zeros(len(edges), dtype=PGO_LINEARIZATION_DTYPE)
        self._check(self.lib.loamx_pose_graph_linearize(self.h, poses.ctypes.data if len(poses) else None, len(poses),
                                                        edges.ctypes.data if len(edges) else None, len(edges), float(huber_delta),
                                                        out.ctypes.data if len(edges) else None))
        return out

    def pose_graph_edges_from_results_dev(self, d_results, d_info, n_pairs, d_edges, first_id=0):
        """the odometry edges (first_id + p, first_id + p + 1) of a sequence's result and information records, on the device"""
        ptr = lambda b: b.ptr if isinstance(b, DeviceBuffer) else b
        self._check(self.lib.loamx_pose_graph_edges_from_results_dev(self.h, ptr(d_results), ptr(d_info), n_pairs, first_id, ptr(d_edges)))

    def synth_scan_pairs_dev(self, seed, first_pair, n_pairs, scan_lines, points_per_line, sigma, d_xyz):
        self._check(self.lib.loamx_synth_scan_pairs_dev(self.h, seed, first_pair, n_pairs, scan_lines,
                                                        points_per_line, sigma, d_xyz))

    # ---- kernel timing --------------------------------------------------------------------------------------
    def enable_kernel_timing(self, on=True):
        self._check(self.lib.loamx_ctx_enable_kernel_timing(self.h, 1 if on else 0))

    def reset_kernel_stats(self):
        self._check(self.lib.loamx_ctx_reset_kernel_stats(self.h))

    def kernel_stats(self):
        st = (KernelStat * K_COUNT)()
        self._check(self.lib.loamx_ctx_get_kernel_stats(self.h, st))
        return {self.lib.loamx_kernel_name(i).decode(): dict(launches=int(st[i].launches), total_ms=st[i].total_ms,
                                                              algorithmic_bytes=st[i].algorithmic_bytes)
                for i in range(K_COUNT)}
