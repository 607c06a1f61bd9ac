/* loamx.h — C ABI of libloamx.so, the MI355X (gfx950) implementation of the two hot paths of
 * DanMcGann/loam: loam::extractFeatures and loam::registerFeatures.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch types. The C++ header
 * shim (the headers under include/loam/), the pybind11 module and bench.py all call through it. Each entry point
 * cites the reference interface it replaces (paths relative to the reference repo root).
 *
 * There is NO CPU fallback: every compute entry point returns LOAMX_ERR_NO_DEVICE / LOAMX_ERR_HIP
 * when no gfx950 device is usable.
 *
 * Conventions
 *   - points: row-major N x 3 FP64 (x,y,z), the layout the reference's Accessors read one by one
 *     (loam/include/loam/common.h:55-78).
 *   - pose: double[7] = {qx, qy, qz, qw, tx, ty, tz}  (Eigen coefficient order, geometry.h:27-31).
 *   - "host" entry points take host pointers and return host results (one scan / one pair);
 *     "_dev" entry points take device pointers, run on the context's stream and do not synchronise.
 */
#ifndef LOAMX_H_
#define LOAMX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct loamx_ctx loamx_ctx;

enum {
  LOAMX_OK = 0,
  LOAMX_ERR_SCAN_SIZE = 1,   /* scan size != scan_lines * points_per_line (common.h:104-113) */
  LOAMX_ERR_BAD_PARAM = 2,
  LOAMX_ERR_HIP = 3,
  LOAMX_ERR_CAPACITY = 4,    /* caller-provided output capacity too small */
  LOAMX_ERR_UNSUPPORTED = 5, /* parameter combination outside what the kernels implement */
  LOAMX_ERR_NO_DEVICE = 6,
  LOAMX_ERR_COMM = 7         /* RCCL error in the multi-GPU gather (loamx_last_error has ncclGetErrorString) */
};

/* loam::LidarParams (loam/include/loam/common.h:29-41) */
typedef struct {
  uint64_t scan_lines;
  uint64_t points_per_line;
  double min_range;
  double max_range;
} loamx_lidar_params;

/* loam::FeatureExtractionParams (loam/include/loam/features.h:37-66): same order, same defaults */
typedef struct {
  uint64_t neighbor_points;             /* 3 */
  uint64_t number_sectors;              /* 6 */
  uint64_t max_edge_feats_per_sector;   /* 10 */
  uint64_t max_planar_feats_per_sector; /* 50 */
  double edge_feat_threshold;           /* 100.0 */
  double planar_feat_threshold;         /* 1.0 */
  double occlusion_thresh;              /* 0.5 */
  double parallel_thresh;               /* 1.0 */
} loamx_fe_params;

/* loam::RegistrationParams (loam/include/loam/registration.h:40-75): same order, same defaults */
typedef struct {
  uint64_t num_edge_neighbors;        /* 5 */
  double max_edge_neighbor_dist;      /* 1.0 */
  uint64_t min_line_fit_points;       /* 3 */
  double min_line_condition_number;   /* 10 */
  uint64_t num_plane_neighbors;       /* 5 */
  double max_plane_neighbor_dist;     /* 2.0 */
  uint64_t min_plane_fit_points;      /* 4 */
  double max_avg_point_plane_dist;    /* 0.1 */
  uint64_t max_iterations;            /* 10 */
  double rotation_convergence_thresh; /* 1e-3 */
  double position_convergence_thresh; /* 1e-2 */
  uint64_t min_associations;          /* 100 */
} loamx_reg_params;

/* loam::RegistrationDetail::TerminationType (registration.h:83) */
enum { LOAMX_CONVERGED = 0, LOAMX_MAX_ITER = 1, LOAMX_INSUFFICIENT_ASSOCIATIONS = 2 };

/* Result of one registration: the returned Pose3d (registration.h:128-131) plus the termination
 * type and the number of ICF iterations executed. 64 bytes; this is the record gathered across
 * ranks in multi-GPU batch mode. */
typedef struct {
  double pose[7];
  uint32_t termination;
  uint32_t iterations;
} loamx_reg_result;

/* One RegistrationDetail::IterationInfo (registration.h:86-104) without the pair lists. */
typedef struct {
  double target_T_source_init[7];
  double estimate_update[7];
  uint32_t n_edge_associations;
  uint32_t n_plane_associations;
} loamx_iter_info;

/* Optional detail capture for loamx_register_features (RegistrationDetail, registration.h:79-109).
 * iter_info: capacity >= params.max_iterations entries. Association pair lists [source idx, nearest
 * target idx] of iteration i are written at edge_pairs + i * 2 * pairs_cap_edge (uint32 pairs) with
 * their count in n_edge_pairs[i] (same for planes); pass NULL pair pointers to skip them. */
typedef struct {
  loamx_iter_info* iter_info;
  uint32_t n_iter_info;   /* out */
  uint32_t* edge_pairs;   /* max_iterations x pairs_cap_edge x 2 */
  size_t pairs_cap_edge;  /* >= number of source edge points */
  uint32_t* n_edge_pairs; /* out, max_iterations entries */
  uint32_t* plane_pairs;
  size_t pairs_cap_plane;
  uint32_t* n_plane_pairs;
} loamx_reg_detail;

void loamx_default_fe_params(loamx_fe_params* p);
void loamx_default_reg_params(loamx_reg_params* p);
const char* loamx_status_string(int status);
const char* loamx_last_error(const loamx_ctx* ctx);

/* Context = one device + one stream + grow-on-demand device workspace. Thread-safe per context. */
int loamx_ctx_create(int device, loamx_ctx** out);
void loamx_ctx_destroy(loamx_ctx* ctx);
/* Use an external hipStream_t; NULL (handle 0) selects the context's OWN private hipStreamNonBlocking stream.
 * Careful with frameworks: torch's default stream has handle 0, i.e. it is NOT adopted — work enqueued by a "_dev"
 * entry point is then ordered only against this context's stream; call loamx_ctx_synchronize (or pass the
 * non-zero handle of an explicit side stream) before another stream or library reads the results. */
int loamx_ctx_set_stream(loamx_ctx* ctx, void* hip_stream);
int loamx_ctx_synchronize(loamx_ctx* ctx);
/* Cumulative counters of the two rare paths of the extraction kernels (synchronises the stream):
 *   tie_replays    scan lines on which two candidates of EQUAL curvature could decide a pick or the output order and
 *                  which were therefore replayed in the order libstdc++'s std::sort gives the reference (features-inl.h:38)
 *   scan_fallbacks calls in which a scan line gave up its (bounded) wait for the lines before it and the features were
 *                  gathered by the fallback kernel instead — the results are the same */
int loamx_ctx_extract_counters(loamx_ctx* ctx, uint64_t* tie_replays, uint64_t* scan_fallbacks);
/* Debug / measurement (no reference counterpart): which kernels the LAST extraction enqueued on this context took —
 * loamx_extract_features*, loamx_compute_curvature / _valid_points, and the extraction inside loamx_register_scan_pairs* /
 * _scan_sequence* (the last chunk's). The bits are set by the launchers at the place where they choose a kernel, not by a
 * second copy of their predicates; a test of "kernel K at shape X" asserts from them that K is what ran. Host side only: no
 * synchronisation, 0 before the first extraction. Never part of a result. */
enum {
  LOAMX_ROUTE_SPLIT_CURV = 1u << 0,     /* curvature handed to the selection as hi words | lo words, validity in the sign bit */
  LOAMX_ROUTE_CURV2 = 1u << 1,          /* curvature_valid2_kernel<3> (two columns per lane) */
  LOAMX_ROUTE_CURV_V1 = 1u << 2,        /* curvature_valid_kernel<3> (option CURV_V1) */
  LOAMX_ROUTE_CURV_GENERIC = 1u << 3,   /* curvature_valid_kernel<0>: neighbor_points as a run-time value */
  LOAMX_ROUTE_ROWS = 1u << 4,           /* select_rows_kernel: four scan lines per wavefront (geometry in the ROWS_R / ROWS_CH fields) */
  LOAMX_ROUTE_ROWS_CH11 = 1u << 5,      /* ... in the instantiation specialised for 11 points per lane; clear: the generic one */
  LOAMX_ROUTE_ROWS_PASS2 = 1u << 6,     /* ... followed by the conditional select_rows_stage_kernel launch (only_if) */
  LOAMX_ROUTE_ROWS_LIST16 = 1u << 7,    /* ... with 16-bit pick lists; clear: bytes */
  LOAMX_ROUTE_MIS = 1u << 8,            /* select_mis_kernel: one scan line per wavefront */
  LOAMX_ROUTE_MIS_4LINES = 1u << 9,     /* ... four lines (wavefronts) per workgroup; clear: one */
  LOAMX_ROUTE_MIS_TWO = 1u << 10,       /* ... two picks per lane (65..128 picks per sector) */
  LOAMX_ROUTE_MIS_CONST_W = 1u << 11,   /* ... with the line length compiled in (1024 / 2048) */
  LOAMX_ROUTE_ARGMAX4 = 1u << 12,       /* select_kernel<4> (arg-max, lines up to 1024 points) */
  LOAMX_ROUTE_ARGMAX1 = 1u << 13,       /* select_kernel<1> (arg-max, longer lines) */
  LOAMX_ROUTE_FUSED_COMPACT = 1u << 14, /* the selection wrote the final arrays itself (compact_kernel only as the conditional fallback) */
  LOAMX_ROUTE_COMPACT = 1u << 15,       /* compact_kernel gathered every scan (unconditional launch) */
  LOAMX_ROUTE_FUSED_EXTRACT = 1u << 16, /* extract_fused_kernel (option FUSED_EXTRACT) */
  LOAMX_ROUTE_FUSED_ROWS = 1u << 17,    /* the fused form of select_rows_kernel (option FUSED_ROWS) */
  LOAMX_ROUTE_BOXES = 1u << 18,         /* the selection's bounding boxes were handed on to the caller (the index builds) */
  LOAMX_ROUTE_ROWS_R_SHIFT = 20,        /* 3 bits: R = neighbor_points - 1 of the row kernels (0 when they did not run) */
  LOAMX_ROUTE_ROWS_CH_SHIFT = 24        /* 6 bits: points of a sector per lane of the row kernels (RowSelGeom::ch) */
};
int loamx_ctx_last_extract_route(loamx_ctx* ctx, uint32_t* bits);
/* Debug / measurement (no reference counterpart): what the solve kernels of the LAST registration enqueued on this context
 * worked on for one of its pairs — which of their record walks a test of "form F at shape X" really ran. Nothing is recorded
 * by the kernels for it: the call synchronises the stream and copies from the workspace the registration wrote anyway, which
 * holds the state of the pair's last completed ICF iteration (a test reads iteration i by running with max_iterations =
 * i + 1 and asking for iterations == i + 1). The source counts are read through the count pointers the call was given: the
 * context's own copies for the host entry points; for the "_dev" entry points the CALLER's arrays, which must still be
 * allocated. Valid from a registration until the next registration, association dump or information call on the context
 * (they size the workspace anew). LOAMX_ERR_BAD_PARAM before any registration and when `pair` is out of range. Never part of
 * a result. */
enum {
  LOAMX_WALK_NONE = 0,           /* no moment pass in that iteration (NO_MOMENTS, or the pair never started a solve): no lists */
  LOAMX_WALK_FLAT = 1,           /* the listed plane records as one flat list in LDS */
  LOAMX_WALK_TILED_BY_COUNT = 2, /* tile by tile: more than flat_cache listed records */
  LOAMX_WALK_TILED_BY_TILES = 3  /* tile by tile: the call's plane capacity makes more than list_cache tiles */
};
typedef struct {
  uint32_t iterations, termination; /* PairState: as in the pair's result record */
  uint32_t use_moments;             /* PairState: the pair's next solve would take the moment pass (0 under NO_MOMENTS) */
  uint32_t mom_ref_on;              /* PairState: the moments were taken at the first candidate (first ICF iteration) ... */
  double mom_ref[7];                /* ... this one */
  uint32_t tiles;                   /* moment tiles per pair of the call: 4 per sweep_chunk slots of plane capacity */
  uint32_t live_tiles;              /* tiles t with (t / 4) * sweep_chunk < n_sp: the ones the kernels look at */
  uint64_t edge_stride, planar_stride; /* slot capacities of the call */
  uint32_t n_se, n_sp;              /* the pair's source counts, clamped to the capacities */
  uint32_t walk;                    /* LOAMX_WALK_*: what the constants below imply for listed_total and tiles */
  uint32_t listed_total;            /* listed plane records (|s| > 0.5 at the reference point) over the live tiles */
  double s0max, v2max;              /* the two maxima behind the moments' validity bound (0 under LOAMX_WALK_NONE) */
  uint32_t sweep_chunk, edge_cache, list_cache, flat_cache; /* the kernels' constants */
  uint32_t* tile_counts;            /* in: room for tile_counts_cap words or NULL; out: listed records of the first */
  size_t tile_counts_cap;           /*     min(live_tiles, tile_counts_cap) live tiles */
} loamx_solve_census;
int loamx_ctx_last_solve_census(loamx_ctx* ctx, size_t pair, loamx_solve_census* out);
/* Debug / measurement (no reference counterpart): the route census of the LAST loamx_associate on this context, for one feature
 * kind (0 = edges, 1 = planes): which kernels the pass launched and how many queries took each route of the k-NN queue chain
 * — what a test of "route R on scene X" really ran. The launch form is noted by the launcher at the branch that chooses it,
 * or computed by the functions the kernels themselves call; the counts come from the workspace, and the two things later
 * kernels overwrite (the count words behind round 1, the counts in front of the queued fit) from a small read-only kernel that
 * ONLY loamx_associate enqueues: no registration or information call launches or records anything for it. Two things stay
 * outside it: the stage at which the brute-force body finished a lane, and the cooperative search's "not applicable" return
 * (a function of the grid, the query's cell distance `out` from the grid and the radius, all reported here:
 * ceil(r / h) + 1 + out > 64 and max(nx, ny, nz) + out > 64). Valid from a loamx_associate until the next registration,
 * association or information call on the context; LOAMX_ERR_BAD_PARAM before any and afterwards. Never part of a result. */
enum { LOAMX_ASSOC_SEARCH_NONE = 0, LOAMX_ASSOC_SEARCH_BRUTE = 1, LOAMX_ASSOC_SEARCH_GRID = 2 }; /* (3: both kernels launched — batches only) */
enum { LOAMX_ASSOC_LEFTOVER_NONE = 0, LOAMX_ASSOC_LEFTOVER_LEFT = 1, LOAMX_ASSOC_LEFTOVER_COOP = 2 };
#define LOAMX_ASSOC_REASON_WIDE 0x80000000u /* bits of entry_reason: round 1 ran out of 8-bit running numbers (a dense block) */
#define LOAMX_ASSOC_REASON_TIED 0x40000000u /* ... its FP32 keys were tied; neither bit: plain (its guard, or outside the grid) */
typedef struct {
  /* launch form */
  uint32_t n_src, n_tgt;       /* queries (clamped to the capacity) and target points of the kind */
  uint64_t stride;             /* slot capacity of the call */
  uint32_t km;                 /* neighbour slots of the kernel instantiation: 5, 8 or 16 (0: the kind was not launched; n_tgt and the grid then read 0) */
  uint32_t search;             /* LOAMX_ASSOC_SEARCH_* */
  uint32_t mixed_launch;       /* first kernels of both kinds as one launch each (associate_knn_mixed_kernel / _fit_mixed_) */
  uint32_t one_stage;          /* queue chain in one stage (0 as well where there is no queue chain: brute force) */
  uint32_t leftover_kernel;    /* LOAMX_ASSOC_LEFTOVER_*: associate_knn_left_kernel or associate_knn_coop_kernel */
  uint32_t rest_blocks, coop_blocks; /* workgroups per pair of the queue kernels / the cooperative kernel (0: not launched) */
  uint32_t rest_spread, left_spread; /* the rest / left kernel dealt its entries across all workgroups (else dense) */
  uint32_t lean_set;           /* the target set is small enough for the lean 5x5x5 search (16-bit positions) */
  double origin[3], h;         /* the target GridDesc */
  int32_t nx, ny, nz;
  uint32_t n_points;
  /* round 1: the count words behind the k-NN (or brute-force) kernel */
  uint32_t verified, unverified, queued_words; /* plain counts / selections for the fit to verify / 0xFFFFFFFF */
  uint32_t queued, queued_plain, queued_wide, queued_tied; /* the queue's length, by the reason bits of its entries */
  /* queue chain */
  uint32_t rest_searched;      /* entries associate_knn_rest_kernel's own condition searches (else handed straight on) */
  uint32_t listed;             /* entries the rest kernel left negative (two stages: listed for the leftover kernel) */
  uint32_t leftover_finished;  /* listed entries the leftover kernel finished */
  uint32_t exact;              /* entries still negative in front of associate_fit_queued_kernel: the exact collector's */
  uint32_t late;               /* selections the fit refused: the late list */
  /* optional, per queue entry: in: room for entries_cap words each or NULL; out: the first min(queued, entries_cap) */
  uint32_t* entry_query;       /* the query: its index in the caller's source array */
  uint32_t* entry_reason;      /* LOAMX_ASSOC_REASON_* */
  int32_t* count_after_rest;   /* count behind associate_knn_rest_kernel (negative: listed) */
  int32_t* count_before_fit;   /* count in front of associate_fit_queued_kernel (negative: exact collector) */
  size_t entries_cap;
  uint32_t* late_query;        /* in: room for late_cap words or NULL; out: the first min(late, late_cap) queries of the late list */
  size_t late_cap;             /*     (indices in the caller's source array, in the list's order) */
} loamx_assoc_census;
int loamx_ctx_last_assoc_census(loamx_ctx* ctx, int which_kind, loamx_assoc_census* out);
/* Beside the census, from the same dump and with the same lifetime: how many listed entries the cooperative leftover kernel gave
 * a row of 16 lanes (out[0]) and how many a whole wavefront (out[1]); counted by the kernel itself where it stores an entry's
 * result, only during an association dump. Both 0 where that kernel was not launched. */
int loamx_ctx_last_assoc_coop_forms(loamx_ctx* ctx, int which_kind, uint32_t out[2]);
/* Debug / measurement switches of ONE context (no reference counterpart). loamx_ctx_create reads the environment
 * variables LOAMX_<NAME> once as the defaults (set = 1); no entry point looks at the environment afterwards, and a
 * switch only ever affects the context it was set on. None changes a result beyond the order in which a pair's residual
 * terms are summed: NO_MOMENTS / NO_REF_MOMENTS (records streamed instead of taken through the moment matrix) and NO_SMALL_SETS
 * (the source edge features are then fed in Morton order instead of the given order: low bits of the pose, asserted by
 * tests/test_gpu_multi.py) — and CHECK_FINITE, which only adds a refusal. For the same reason the default results of two
 * RELEASES may differ in the low bits (far below the 1e-5 parity bar): round 5 began to feed the source edge features of a
 * pair whose target edge set has at most 512 points in their given order. Names — the complete list; DESIGN.md section 5:
 *   extraction:    FORCE_TIE_REPLAY, FORCE_SCAN_GIVEUP, CURV_V1, NO_FUSED_COMPACT, NO_MIS_SELECT, NO_ROW_SELECT, FUSED_EXTRACT,
 *                  FUSED_ROWS, NO_SPLIT_CURV, STAGE_ALWAYS
 *   registration:  NO_MOMENTS, NO_REF_MOMENTS, NO_PACKED_GRID, NO_BIG_GRID, NO_GRID_SIDE, NO_EXTRACT_BOXES, NO_SMALL_SETS, DEBUG_POISON,
 *                  QUEUE_TWO_STAGE, QUEUE_ONE_STAGE, NO_COOP_LEFT, NO_COOP_ROWS, NO_MIXED_ASSOC, FORCE_LATE_VERIFY, NO_LIVE_DEAL, MAP_CELLS_LOG2 (a number: 0 = default)
 *   host streaming: STREAM_CHUNK_PAIRS (a number: pairs per uploaded chunk of loamx_register_scan_pairs / _scan_sequence; 0 = default, 128)
 *   multi-GPU:     FORCE_RCCL (a one-rank communicator really enqueues the RCCL collectives)
 *   input checks:  CHECK_FINITE (see "Non-finite input" below)
 *   cloud map:     NO_CLOUDMAP_COMBINE (one claim per point instead of one per run of a wavefront: the same bytes, see "cloud map")
 *   segmentation:  NO_SEGMENT_TILES (every connected edge through the global union, no tile labelling in LDS: the same bytes, see "scan segmentation")
 *   map cleaning:  NO_VISIBILITY_RANGES (the votes kernel reads the scans' points, no first launch that writes every cell's squared range: the same bytes, see "map cleaning")
 *   occupancy map: NO_OCCUPANCY_COMBINE (one claim per visit instead of one per run of a wavefront: the same bytes, see "occupancy map")
 *   distance field: NO_DISTANCE_EARLY_EXIT (the y- and z-pass walk their whole window: the same bytes, see "occupancy distance field")
 *   ray casting:   RAYCAST_COMBINE (one look-up per run of neighbouring lanes in the same voxel instead of one per lane: the same bytes, see "occupancy ray casting")
 *   surfel map:    NO_SURFEL_COMBINE (one claim per point instead of one per run of a wavefront: the same bytes, see "surfel map")
 *   localisation:  NO_LOCALIZE_PLANES (no plane cache, every candidate voxel finished where it is looked at: the same bytes, see "surfel localisation")
 * Unknown name: LOAMX_ERR_BAD_PARAM.
 *
 * Non-finite input. The reference is undefined on NaN / Inf coordinates (loam/include/loam/features-inl.h:38 sorts on
 * curvatures computed from them; a NaN range passes every comparison of loam/src/features.cpp:30-68; nanoflann and Ceres
 * receive them as they are). Here: every HOST entry point (loamx_compute_curvature / _valid_points, loamx_extract_features,
 * loamx_register_features / _indexed, loamx_register_scan_pairs, loamx_register_scan_sequence, loamx_associate, loamx_fit_lines / _planes, loamx_knn_search, loamx_target_index_create /
 * _insert / _insert_filtered (points and pose), and their _f32 forms) refuses such input with LOAMX_ERR_BAD_PARAM: its uploaded copy is looked at by one small
 * kernel before anything else is launched (a 4-byte read-back, one extra stream synchronisation; an index is left as it was). The "_dev" entry points (loamx_extract_features_batch_dev, loamx_register_features_batch_dev,
 * loamx_register_scan_pairs_dev, loamx_register_scan_sequence_dev, and their _f32 forms) do not look unless the context option CHECK_FINITE is set: then one
 * small kernel and a 4-byte read-back precede the call (it synchronises) and non-finite input is refused the same way.
 * Without it their result on such input is unspecified, as the reference's. */
int loamx_ctx_set_option(loamx_ctx* ctx, const char* name, int value);
int loamx_ctx_get_option(loamx_ctx* ctx, const char* name, int* value);

/* ---- host entry points (one scan / one pair; H2D, kernels, D2H, synchronous) ------------------ */

/* loam::computeCurvature (features.h:119-122, features-inl.h:53-87): curvature_out[n_points] */
int loamx_compute_curvature(loamx_ctx* ctx, const double* xyz, size_t n_points, const loamx_lidar_params* lidar,
                            const loamx_fe_params* fe, double* curvature_out);
/* loam::computeValidPoints (features.h:166-169, features-inl.h:90-124): mask_out[n_points] in {0,1} */
int loamx_compute_valid_points(loamx_ctx* ctx, const double* xyz, size_t n_points,
                               const loamx_lidar_params* lidar, const loamx_fe_params* fe, uint8_t* mask_out);
/* loam::extractFeatures (features.h:108-111, features-inl.h:11-50). Writes the indices of the edge
 * and planar feature points in the reference's output order; the caller copies the points
 * (the C++ shim does, reproducing LoamFeatures). Capacity needed: scan_lines * number_sectors *
 * (max_*_feats_per_sector + 1). */
int loamx_extract_features(loamx_ctx* ctx, const double* xyz, size_t n_points, const loamx_lidar_params* lidar,
                           const loamx_fe_params* fe, uint32_t* edge_idx, size_t edge_cap, size_t* n_edge,
                           uint32_t* planar_idx, size_t planar_cap, size_t* n_planar);
/* FP32-input twins: xyz as n_points x 3 floats, e.g. PCL points. The reference's FieldAccessor
 * (common.h:55-60) widens every coordinate to double before any arithmetic; the kernels do the same on load,
 * so the results are those of the FP64 entry points on the widened values, bit for bit, at half the input bytes. */
int loamx_compute_curvature_f32(loamx_ctx* ctx, const float* xyz, size_t n_points, const loamx_lidar_params* lidar,
                                const loamx_fe_params* fe, double* curvature_out);
int loamx_compute_valid_points_f32(loamx_ctx* ctx, const float* xyz, size_t n_points,
                                   const loamx_lidar_params* lidar, const loamx_fe_params* fe, uint8_t* mask_out);
int loamx_extract_features_f32(loamx_ctx* ctx, const float* xyz, size_t n_points, const loamx_lidar_params* lidar,
                               const loamx_fe_params* fe, uint32_t* edge_idx, size_t edge_cap, size_t* n_edge,
                               uint32_t* planar_idx, size_t planar_cap, size_t* n_planar);
/* loam::registerFeatures (registration.h:128-131, registration-inl.h:11-78). detail may be NULL.
 * Every entry point that takes a loamx_reg_params answers LOAMX_ERR_UNSUPPORTED for num_*_neighbors > 16 and for
 * max_iterations > 1000, and LOAMX_ERR_BAD_PARAM for min_line_fit_points < 2 or min_plane_fit_points < 3 while that kind's
 * num_*_neighbors is above 0; min_*_fit_points above 64 count as 64 and min_associations above 2^32 - 1 as 2^32 - 1.
 * max_avg_point_plane_dist is compared with a value that is never positive: the gate acts below 0 only. */
int loamx_register_features(loamx_ctx* ctx, const double* src_edge, size_t n_src_edge, const double* src_planar,
                            size_t n_src_planar, const double* tgt_edge, size_t n_tgt_edge,
                            const double* tgt_planar, size_t n_tgt_planar, const double init_pose[7],
                            const loamx_reg_params* reg, loamx_reg_result* result, loamx_reg_detail* detail);

/* ---- persistent target index (scan-to-map; the reference rebuilds both KD-trees on every
 * call, registration-inl.h:20-23). Build the spatial index of a target feature set (e.g. a local map)
 * once, keep it resident on the device and register any number of source scans against it.
 * The index depends on max_edge_neighbor_dist / max_plane_neighbor_dist of `reg` (cell size);
 * loamx_register_features_indexed fails with LOAMX_ERR_BAD_PARAM if they differ. */
typedef struct loamx_target_index loamx_target_index;
int loamx_target_index_create(loamx_ctx* ctx, const double* tgt_edge, size_t n_tgt_edge, const double* tgt_planar,
                              size_t n_tgt_planar, const loamx_reg_params* reg, loamx_target_index** out);
void loamx_target_index_destroy(loamx_ctx* ctx, loamx_target_index* index);
/* Appends points to the index (a map that grows scan by scan). The new points take the indices that follow the
 * existing ones, and every search and registration against the index afterwards returns what it would against an
 * index created over the concatenated sets, bit for bit (the searches are exact: their result does not depend on
 * the cell structure). Cost: one upload of the NEW points, then per feature kind either
 *   - a merge into the existing grid (map-sized kinds: counts and scatter of the new points, one table scan and one
 *     streaming copy of the cell-sorted arrays into their twin buffers: ~0.1 ms per million resident points), or
 *   - a rebuild of that kind (scan-sized kinds: one workgroup; any kind when a new point lies outside its grid, when
 *     the kind has doubled since its grid was chosen — the cell edge follows the density — or when its buffers grew).
 * Amortised over a map grown scan by scan the rebuilds are O(log n) events. */
int loamx_target_index_insert(loamx_ctx* ctx, loamx_target_index* index, const double* edge, size_t n_edge,
                              const double* planar, size_t n_planar);
/* how the index has been maintained so far: full (re)builds of a feature kind's grid (counted per kind: creating an index
 * with both kinds counts two) / merges into an existing one. A kind that receives no points in an insert is left alone. */
int loamx_target_index_stats(const loamx_target_index* index, uint64_t* full_builds, uint64_t* merges);
/* number of edge / planar points in the index (either pointer may be NULL) */
int loamx_target_index_size(const loamx_target_index* index, size_t* n_edge, size_t* n_planar);
/* Debug / measurement (no reference counterpart): one feature kind of a persistent index as it lies on the device, and which
 * form of the index build made it — what a test of "build form F at shape X" asserts instead of assuming. `build`, the unit
 * behind lds_passes / scan_tiles and the rule behind table_valid are recorded by the launcher at the place where it chooses
 * the kernel, never derived from a second copy of its predicates (the rule of LOAMX_ROUTE_* above). Nothing is recorded by the
 * kernels: the call synchronises the stream and copies from the index's own arrays. Never part of a result.
 * LOAMX_ERR_BAD_PARAM: which_set not 0 / 1, a kind whose grid is not valid (a failed insert), a buffer too small. */
enum {
  LOAMX_INDEX_BUILD_NONE = 0,
  LOAMX_INDEX_BUILD_PACKED = 1, /* grid_build_kernel<false, true>: one workgroup, 16-bit cell counters, cell order in LDS */
  LOAMX_INDEX_BUILD_SINGLE = 2, /* grid_build_kernel<false, false>: one workgroup, 32-bit counters (NO_PACKED_GRID / NO_BIG_GRID) */
  LOAMX_INDEX_BUILD_BIG = 3     /* the multi-workgroup gridbig_* kernels */
};
enum { LOAMX_INDEX_OP_NONE = 0, LOAMX_INDEX_OP_FULL_BUILD = 1, LOAMX_INDEX_OP_MERGE = 2 };
typedef struct {
  uint64_t n, capacity;          /* points of the kind / points its buffers hold without growing (the builds are chosen by it) */
  double origin[3], h, inv_h;    /* the GridDesc, copied from the device */
  int32_t nx, ny, nz;
  uint32_t n_points;
  uint32_t build;                /* LOAMX_INDEX_BUILD_*: the form of the kind's last FULL build */
  uint32_t table_valid;          /* 0: that build left the cell table unwritten (single-workgroup forms, sets of at most 512 points) */
  uint64_t table_entries;        /* capacity of the cell table: 65 536, or the map table's */
  uint32_t lds_passes;           /* PACKED / SINGLE: ceil(nx ny nz / cells per LDS pass), else 0 */
  uint32_t scan_tiles;           /* BIG: ceil(nx ny nz / entries per scan tile), else 0 */
  uint32_t last_op, reserved;    /* LOAMX_INDEX_OP_*: what brought the kind to its present state */
  uint64_t full_builds, merges;  /* of THIS kind (loamx_target_index_stats counts both kinds together) */
  /* optional copies, NULL to skip; a capacity below the need is LOAMX_ERR_BAD_PARAM */
  uint32_t* cell_start;          /* [nx ny nz + 1]; left untouched while table_valid == 0 */
  size_t cell_start_cap;
  double* xyz;                   /* [n][3] the cell-sorted points ... */
  uint32_t* orig;                /* [n]    ... and their indices in insertion order */
  size_t points_cap;
  float* rel;                    /* [3][rel_cap]: the first n + 4 entries of each plane (the four pad entries included) */
  size_t rel_cap;
} loamx_index_census;
int loamx_target_index_census(loamx_ctx* ctx, const loamx_target_index* index, int which_set, loamx_index_census* out);
/* same contract as loamx_register_features, target taken from the index */
int loamx_register_features_indexed(loamx_ctx* ctx, const loamx_target_index* index, const double* src_edge,
                                    size_t n_src_edge, const double* src_planar, size_t n_src_planar,
                                    const double init_pose[7], const loamx_reg_params* reg, loamx_reg_result* result,
                                    loamx_reg_detail* detail);

/* ---- map upkeep (no reference counterpart: the reference registers scan to scan and leaves the map to its users). What a
 * LOAM mapper does after every registration, on the device: move the scan's features into the map frame, thin them on a
 * voxel grid so that a slow or standing vehicle does not pile points into the same cells, add them, and drop what has left
 * the local window.
 *   transform  p' = pose.act(p) with the arithmetic of the association's *_moved (Pose3d::act; the quaternion is used as given,
 *              not normalised). An identity pose (NULL, or exactly {0,0,0,1,0,0,0}) returns the input bit for bit.
 *   voxel      v[c] = floor(p'[c] / leaf) (an IEEE FP64 division, so a point on a voxel face lands where numpy.floor(p / leaf)
 *              puts it); |v[c]| < 2^20; key = (v.x + 2^20) << 42 | (v.y + 2^20) << 21 | (v.z + 2^20).
 *   kept set   of all points of a call that share a voxel the one with the LOWEST input index is kept — for an index, only if
 *              no point of the map lies in that voxel; the kept points leave in input order. The result does not depend on
 *              how the threads are scheduled: two runs give the same bytes. */

/* Points first .. first + count - 1 of one set (which_set: 0 edge, 1 planar) in index order, to HOST memory. first + count
 * beyond the set: LOAMX_ERR_BAD_PARAM; count == 0: LOAMX_OK. */
int loamx_target_index_points(loamx_ctx* ctx, const loamx_target_index* index, int which_set, size_t first, size_t count,
                              double* xyz_out);
/* Transform + voxel filter of n DEVICE points; pose: HOST pointer, NULL = identity. d_n_out: the number kept; d_xyz_out[j]
 * (room for n points): the j-th kept point, transformed; d_src_idx[j] (n entries, may be NULL): its input index; entries past
 * the count are unspecified. leaf <= 0: no filter — every point is kept and the call is the transform alone. Otherwise a
 * point with a non-finite coordinate or a voxel coordinate out of range is dropped. d_xyz_out == d_xyz, a NaN leaf or a
 * non-finite pose: LOAMX_ERR_BAD_PARAM (any other overlap is undefined); n == 0 writes a zero count. Asynchronous on the
 * context's stream. */
int loamx_voxel_filter_dev(loamx_ctx* ctx, const double* d_xyz, size_t n, const double pose[7], double leaf, double* d_xyz_out,
                           uint32_t* d_src_idx, uint32_t* d_n_out);
/* loamx_target_index_insert of the points the voxel filter keeps: p' = world_T_scan.act(p) (NULL = identity) is added unless
 * its voxel already holds a point of the map — however that point got there: at create, by a plain or by a filtered insert;
 * judged at this call's leaf — or an earlier point of this call. The index afterwards is, byte for byte, what
 * loamx_target_index_insert of exactly the kept points makes of it (merges, rebuilds and the counters of
 * loamx_target_index_stats included); a kind to which the call adds nothing is left alone. A kind whose leaf is <= 0 is
 * transformed and inserted unfiltered. n_*_added (either may be NULL): points added per kind. Non-finite points or pose, or
 * a NaN leaf: LOAMX_ERR_BAD_PARAM; a point (of the call, or of the map at this leaf) whose voxel is out of range:
 * LOAMX_ERR_UNSUPPORTED; the index stays as it was. Each kind keeps an occupancy table (12 B per slot, 2 - 6 slots per map
 * point) built by the first filtered insert, so later calls hash the new points only; it is built again when the leaf
 * differs from the last call's, when the map has outgrown it, and after a crop. */
int loamx_target_index_insert_filtered(loamx_ctx* ctx, loamx_target_index* index, const double* edge, size_t n_edge,
                                       const double* planar, size_t n_planar, const double world_T_scan[7], double edge_leaf,
                                       double planar_leaf, size_t* n_edge_added, size_t* n_planar_added);
/* Keeps the points with lo[c] <= p[c] <= hi[c] for c = x, y, z; the survivors keep their relative order, and the index
 * afterwards equals one created over them. A kind that loses points is rebuilt (counted as a full build), a kind that loses
 * none is not touched; a kind may become empty. n_*_removed: either may be NULL. lo[c] > hi[c] or a NaN bound:
 * LOAMX_ERR_BAD_PARAM; infinite bounds are allowed. */
int loamx_target_index_crop(loamx_ctx* ctx, loamx_target_index* index, const double lo[3], const double hi[3],
                            size_t* n_edge_removed, size_t* n_planar_removed);

/* ---- rows a16-a19 one by one (round 3): the reference's internal functions behind registerFeatures, callable from the
 * host. Same device functions the association kernels run; used by the header shim's geometry_internal / kdtree_internal
 * namespaces and by the parity tests that compare neighbour lists and fits with the oracle directly. ------------------ */

/* geometry_internal::fitLine (geometry.h:102, geometry.cpp:42-59) for n_sets point sets of k points each
 * (points: n_sets x k x 3 doubles, 2 <= k <= 32). lines_out: n_sets x 6 = {a, b} with a = centre + 0.1 dir,
 * b = centre - 0.1 dir; cond_out (may be NULL): the condition number the reference returns, i.e. DBL_MAX always
 * (geometry.cpp:55-56 computes the ratio and drops it). */
int loamx_fit_lines(loamx_ctx* ctx, const double* points, size_t n_sets, size_t k, double* lines_out, double* cond_out);
/* geometry_internal::fitPlane (geometry.h:123, geometry.cpp:62-73), 3 <= k <= 32. planes_out: n_sets x 4 = {normal, d};
 * avg_dist_out (may be NULL): the signed mean of P n - d. */
int loamx_fit_planes(loamx_ctx* ctx, const double* points, size_t n_sets, size_t k, double* planes_out, double* avg_dist_out);
/* kdtree_internal::knnSearch (kdtree.h:49, kdtree.cpp:10-28) for n_queries points against one set of a target index
 * (which_set: 0 = its edge points, 1 = its planar points; the index plays the role of the reference's KDTree):
 * exact k nearest (k <= 16), ascending, then the strict radius filter (max_dist <= 0: none). indices_out:
 * n_queries x k indices into the array the index was built from (0xFFFFFFFF past the count); counts_out: n_queries. */
int loamx_knn_search(loamx_ctx* ctx, const loamx_target_index* index, int which_set, const double* queries, size_t n_queries,
                     size_t k, double max_dist, uint32_t* indices_out, uint32_t* counts_out);
/* registration_internal::associateEdges / associatePlanes (registration.h:205-222, registration.cpp:23-103) at a given
 * estimate: ONE association pass of the registration kernels themselves (index builds, round-1 k-NN, queue chain,
 * fits), read out per source feature instead of being handed to the solver. Any pointer may be NULL (skipped).
 *   *_nn_count  n_src          neighbours that passed the radius filter (kdtree.cpp:25)
 *   *_nn_idx    n_src x k      their indices in the target array, ascending distance (0xFFFFFFFF past the count)
 *   *_valid     n_src          1: the reference would add a residual block for this point (all guards passed)
 *   *_moved     n_src x 3      pose.act(source point) (registration.cpp:34 / :75)
 *   edge_lines  n_src x 6      fitted line {a, b};  plane_planes  n_src x 4  {normal, d}   (when >= min_*_fit_points) */
typedef struct {
  uint32_t* edge_nn_count;
  uint32_t* edge_nn_idx;
  uint8_t* edge_valid;
  double* edge_moved;
  double* edge_lines;
  uint32_t* plane_nn_count;
  uint32_t* plane_nn_idx;
  uint8_t* plane_valid;
  double* plane_moved;
  double* plane_planes;
  uint32_t* queue_lengths; /* 4: queries the first k-NN pass handed on {edge, plane}, then those its second pass handed on */
} loamx_assoc_dump;
int loamx_associate(loamx_ctx* ctx, const double* src_edge, size_t n_src_edge, const double* src_planar, size_t n_src_planar,
                    const double* tgt_edge, size_t n_tgt_edge, const double* tgt_planar, size_t n_tgt_planar,
                    const double pose[7], const loamx_reg_params* reg, loamx_assoc_dump* out);

/* ---- registration information matrix (no reference counterpart: the reference returns a pose and nothing else) ----------
 * The 6x6 Gauss-Newton information matrix H = sum J^T J of the registration residuals of a pair at a pose T = target_T_source,
 * with its eigen-decomposition: what a pose graph or a filter needs next to the pose (a covariance), and what LOAM's mapping
 * thread, LeGO-LOAM and LIO-SAM threshold to detect corridors, tunnels and open fields (the small eigenvalues and their
 * directions). The pair is associated ONCE at T, exactly as loamx_associate does (same kernels, same parameters of
 * loamx_reg_params; max_iterations, the convergence thresholds and min_associations play no part, max_iterations == 0 is
 * fine). Every valid association with moved point v = T.act(p) contributes one row:
 *   plane  s = n.v - d,             r = |s|,           g = copysign(1, s) n
 *   edge   c = (v - a) x (v - b),   r = |c| / |a - b|, g = ((a - b) x c) / (|c| |a - b|)
 *   row    J = [ v x g , g ]  (1 x 6): the derivative of r for the LEFT perturbation T <- Exp([omega, t]) o T, omega a rotation
 *          vector in radians about the TARGET frame's axes, t in metres, rotation first (columns 0-2 omega, 3-5 t)
 *   Huber(1.0) as the solver applies it: for r^2 > 1, J and r are scaled by sqrt(1 / r)
 *   a row with a non-finite entry is left out and counted in n_dropped (an edge point exactly on its line has |c| = 0)
 * A pair without a single row gives a zero matrix, zero eigenvalues and identity eigenvectors. Deterministic: the same bytes
 * on every run, and the same bytes for a pair whether it is computed alone or inside any batch (fixed chunks of a pair's
 * association slots, partial sums added in chunk order). Records are per rank: the multi-GPU gather does not carry them. */
typedef struct {
  double information[36];   /* H = sum J^T J, row-major, bitwise symmetric */
  double eigenvalues[6];    /* ascending */
  double eigenvectors[36];  /* row i: unit eigenvector of eigenvalues[i]; its largest-magnitude component (lowest index on ties) is positive */
  double gradient[6];       /* sum J^T r  (scaled rows and residuals) */
  double weighted_sq_error; /* sum of scaled r^2 */
  uint32_t n_edge, n_plane; /* rows that entered the sums */
  uint32_t n_huber;         /* of those, rows with r^2 > 1 */
  uint32_t n_dropped;       /* valid associations left out (non-finite row) */
} loamx_reg_information;    /* 696 bytes */
/* host, one pair (H2D, kernels, D2H, synchronous). Null pointers, non-finite points or pose: LOAMX_ERR_BAD_PARAM;
 * num_*_neighbors > 16: LOAMX_ERR_UNSUPPORTED — as loamx_register_features. */
int loamx_registration_information(loamx_ctx* ctx, const double* src_edge, size_t n_src_edge, const double* src_planar,
                                   size_t n_src_planar, const double* tgt_edge, size_t n_tgt_edge, const double* tgt_planar,
                                   size_t n_tgt_planar, const double pose[7], const loamx_reg_params* reg,
                                   loamx_reg_information* info);
/* the same against a persistent target index (scan-to-map: where degeneracy matters most) */
int loamx_registration_information_indexed(loamx_ctx* ctx, const loamx_target_index* index, const double* src_edge,
                                           size_t n_src_edge, const double* src_planar, size_t n_src_planar, const double pose[7],
                                           const loamx_reg_params* reg, loamx_reg_information* info);

/* ---- device-resident batch entry points (asynchronous on the context stream) ------------------ */

/* Feature buffers of scan s live at base + s * stride with
 *   edge stride   = loamx_edge_capacity(lidar, fe)   entries,
 *   planar stride = loamx_planar_capacity(lidar, fe) entries. */
size_t loamx_edge_capacity(const loamx_lidar_params* lidar, const loamx_fe_params* fe);
size_t loamx_planar_capacity(const loamx_lidar_params* lidar, const loamx_fe_params* fe);

/* extractFeatures over n_scans scans stored back to back (d_xyz: n_scans x N x 3 doubles).
 * d_*_idx: uint32 indices into the scan; d_*_xyz: copies of the points (may be NULL);
 * d_n_edge / d_n_planar: one uint32 count per scan. */
int loamx_extract_features_batch_dev(loamx_ctx* ctx, const double* d_xyz, size_t n_scans,
                                     const loamx_lidar_params* lidar, const loamx_fe_params* fe,
                                     uint32_t* d_edge_idx, uint32_t* d_n_edge, double* d_edge_xyz,
                                     uint32_t* d_planar_idx, uint32_t* d_n_planar, double* d_planar_xyz);

/* the same over float scans (d_xyz: n_scans x N x 3 floats); the point copies are FP64 (widened) */
int loamx_extract_features_batch_dev_f32(loamx_ctx* ctx, const float* d_xyz, size_t n_scans,
                                         const loamx_lidar_params* lidar, const loamx_fe_params* fe,
                                         uint32_t* d_edge_idx, uint32_t* d_n_edge, double* d_edge_xyz,
                                         uint32_t* d_planar_idx, uint32_t* d_n_planar, double* d_planar_xyz);

/* registerFeatures over n_pairs independent pairs. Feature set f of pair p: points at
 * d_*[p * stride * 3], count d_n_*[p]. d_init: n_pairs x 7 doubles or NULL (identity). */
int loamx_register_features_batch_dev(loamx_ctx* ctx, size_t n_pairs, const double* d_src_edge,
                                      const uint32_t* d_n_src_edge, const double* d_src_planar,
                                      const uint32_t* d_n_src_planar, const double* d_tgt_edge,
                                      const uint32_t* d_n_tgt_edge, const double* d_tgt_planar,
                                      const uint32_t* d_n_tgt_planar, size_t edge_stride, size_t planar_stride,
                                      const double* d_init, const loamx_reg_params* reg,
                                      loamx_reg_result* d_results);

/* loamx_registration_information over n_pairs independent pairs: the argument list of loamx_register_features_batch_dev with
 * the poses d_pose (n_pairs x 7 doubles, NULL = identity) in place of d_init and one information record per pair in place of
 * the results. */
int loamx_registration_information_batch_dev(loamx_ctx* ctx, size_t n_pairs, const double* d_src_edge,
                                             const uint32_t* d_n_src_edge, const double* d_src_planar,
                                             const uint32_t* d_n_src_planar, const double* d_tgt_edge,
                                             const uint32_t* d_n_tgt_edge, const double* d_tgt_planar,
                                             const uint32_t* d_n_tgt_planar, size_t edge_stride, size_t planar_stride,
                                             const double* d_pose, const loamx_reg_params* reg,
                                             loamx_reg_information* d_info);

/* The north-star unit: one scan-pair registration = extractFeatures(target scan), extractFeatures(
 * source scan), registerFeatures(source, target, identity). d_xyz holds n_pairs x 2 scans, target
 * scan first. Results are device resident. */
int loamx_register_scan_pairs_dev(loamx_ctx* ctx, const double* d_xyz, size_t n_pairs,
                                  const loamx_lidar_params* lidar, const loamx_fe_params* fe,
                                  const loamx_reg_params* reg, loamx_reg_result* d_results);

/* The same unit from HOST memory to host memory — the reference's own unit of use (README.md:44-60: a scan pair in host
 * memory in, a pose out). The batch is cut into chunks of `STREAM_CHUNK_PAIRS` pairs (context option, a number; 0 = the
 * default, 128); chunk k + 1 travels to the device on a copy stream (hipMemcpyAsync into the second of two staging buffers)
 * while chunk k is registered through loamx_register_scan_pairs_dev's own path; the 64-byte results come back in one copy at
 * the end. Results are bit-identical to the "_dev" entry point's. For the upload to overlap the kernels `xyz` must be pinned
 * (hipHostMalloc / hipHostRegister); pageable memory works, one chunk at a time. Throughput is PCIe's: 3.1 MB of FP64 scans
 * per pair (1.6 MB as floats) against ~10 us of kernels. Non-finite input is refused (LOAMX_ERR_BAD_PARAM) chunk by chunk. */
int loamx_register_scan_pairs(loamx_ctx* ctx, const double* xyz, size_t n_pairs, const loamx_lidar_params* lidar,
                              const loamx_fe_params* fe, const loamx_reg_params* reg, loamx_reg_result* results);
int loamx_register_scan_pairs_f32(loamx_ctx* ctx, const float* xyz, size_t n_pairs, const loamx_lidar_params* lidar,
                                  const loamx_fe_params* fe, const loamx_reg_params* reg, loamx_reg_result* results);

/* the same over float scans */
int loamx_register_scan_pairs_dev_f32(loamx_ctx* ctx, const float* d_xyz, size_t n_pairs,
                                      const loamx_lidar_params* lidar, const loamx_fe_params* fe,
                                      const loamx_reg_params* reg, loamx_reg_result* d_results);

/* ---- scan sequences ------------------------------------------------------------------------------------------
 * The reference's own use (README.md, "Example Usage") is a loop over a sensor stream: scan i is the source of one
 * registration and the target of the next. These entry points take n_scans consecutive scans stored back to back and
 * register the n_scans - 1 consecutive pairs: pair p has scan p as target and scan p + 1 as source, results[p].pose is
 * target_T_source exactly as in loamx_register_scan_pairs_dev, and every scan is extracted ONCE (the pair entry points,
 * fed the duplicated layout [(scan p, scan p + 1)], upload and extract every interior scan twice). The records are bit-identical
 * to the pair entry points' on that duplicated layout. d_init / init: (n_scans - 1) x 7 doubles, the initial
 * target_T_source of every pair, or NULL (identity). n_scans < 2: LOAMX_OK, nothing is written. Parameter checks, the
 * non-finite refusal and the error codes are those of the pair entry points (the initial poses are looked at with the scans).
 *
 * Host form: the pairs are cut into chunks of STREAM_CHUNK_PAIRS pairs (default 128) as in loamx_register_scan_pairs; chunk
 * k of C pairs uploads the C + 1 scans it reads, so the scan two neighbouring chunks share travels and is extracted twice
 * (1 / C extra): (C + 1) / C scans per pair cross PCIe instead of 2.
 * Multi-GPU: shard the PAIRS with loamx_shard_range; rank r reads scans [first, first + count] (count + 1 of them) and the
 * gather of the records is unchanged. */
int loamx_register_scan_sequence_dev(loamx_ctx* ctx, const double* d_xyz, size_t n_scans, const loamx_lidar_params* lidar,
                                     const loamx_fe_params* fe, const loamx_reg_params* reg, const double* d_init,
                                     loamx_reg_result* d_results);
int loamx_register_scan_sequence_dev_f32(loamx_ctx* ctx, const float* d_xyz, size_t n_scans, const loamx_lidar_params* lidar,
                                         const loamx_fe_params* fe, const loamx_reg_params* reg, const double* d_init,
                                         loamx_reg_result* d_results);
int loamx_register_scan_sequence(loamx_ctx* ctx, const double* xyz, size_t n_scans, const loamx_lidar_params* lidar,
                                 const loamx_fe_params* fe, const loamx_reg_params* reg, const double* init,
                                 loamx_reg_result* results);
int loamx_register_scan_sequence_f32(loamx_ctx* ctx, const float* xyz, size_t n_scans, const loamx_lidar_params* lidar,
                                     const loamx_fe_params* fe, const loamx_reg_params* reg, const double* init,
                                     loamx_reg_result* results);
/* The "_dev" pair and sequence entry points with the information matrix behind the registration: d_results as the plain
 * forms write them (bit-identical), plus d_info[p] = the information record of pair p taken at d_results[p].pose — one more
 * association pass at the final poses against the target indexes the registration built, then the two information kernels.
 * The records are those of loamx_registration_information_batch_dev at these poses on the pairs' extracted features. */
int loamx_register_scan_pairs_info_dev(loamx_ctx* ctx, const double* d_xyz, size_t n_pairs, const loamx_lidar_params* lidar,
                                       const loamx_fe_params* fe, const loamx_reg_params* reg, loamx_reg_result* d_results,
                                       loamx_reg_information* d_info);
int loamx_register_scan_pairs_info_dev_f32(loamx_ctx* ctx, const float* d_xyz, size_t n_pairs, const loamx_lidar_params* lidar,
                                           const loamx_fe_params* fe, const loamx_reg_params* reg, loamx_reg_result* d_results,
                                           loamx_reg_information* d_info);
int loamx_register_scan_sequence_info_dev(loamx_ctx* ctx, const double* d_xyz, size_t n_scans, const loamx_lidar_params* lidar,
                                          const loamx_fe_params* fe, const loamx_reg_params* reg, const double* d_init,
                                          loamx_reg_result* d_results, loamx_reg_information* d_info);
int loamx_register_scan_sequence_info_dev_f32(loamx_ctx* ctx, const float* d_xyz, size_t n_scans, const loamx_lidar_params* lidar,
                                              const loamx_fe_params* fe, const loamx_reg_params* reg, const double* d_init,
                                              loamx_reg_result* d_results, loamx_reg_information* d_info);
/* The chained trajectory of n_pairs consecutive results (device records): d_world_T_scan holds (n_pairs + 1) x 7 doubles,
 * world_T_scan[0] = origin (HOST pointer to a pose; NULL = identity), world_T_scan[i + 1] = world_T_scan[i] (+) results[i].pose
 * with the arithmetic of Pose3d::compose (geometry.h:32), in the order of the loop a host would write — a pair that ended
 * LOAMX_INSUFFICIENT_ASSOCIATIONS contributes the pose it returned, as in that loop. Deterministic: the same bytes on every
 * run. Asynchronous on the context's stream. */
int loamx_compose_trajectory_dev(loamx_ctx* ctx, const loamx_reg_result* d_results, size_t n_pairs, const double origin[7],
                                 double* d_world_T_scan);
/* Motion correction ("de-skew", the dewarping step the reference's README leaves to its users) of n_scans scans stored back
 * to back. Scans are row-major [line][column]; column c was measured at sweep fraction tau = c / points_per_line.
 * d_motion[s] = {qx, qy, qz, qw, tx, ty, tz} is start_T_end of sweep s: the sensor's pose at the end of the sweep in its
 * frame at the start (for consecutive sweeps at constant velocity: the previous pair's target_T_source). q is normalised and
 * taken along the short arc (negated if w < 0). With T(tau) = (slerp(identity, q, tau), tau t) a point becomes
 *     p_out = R(rho)^T (R(tau) p + (tau - rho) t),   rho = ref_fraction in [0, 1] (otherwise LOAMX_ERR_BAD_PARAM):
 * the point in the sensor frame at fraction rho. rho = 1 is the end of the sweep (LOAM's convention), rho = 0 its start.
 * All arithmetic is FP64; the f32 form widens on load and rounds once on store. An identity motion returns the input bit for
 * bit. A point whose three coordinates are all exactly zero (a beam without a return) stays zero and a point with a
 * non-finite coordinate is copied unchanged, so the output is a scan like the input. d_xyz_out may equal d_xyz (in place);
 * any other overlap is undefined. Asynchronous on the context's stream; lidar->min_range / max_range are not used.
 * The motion quaternion must have a norm within [1e-150, 1e150] (it need not be a unit quaternion). Outside that range the
 * squares of its components underflow or overflow; a zero quaternion, or one whose squares underflow to 0, has no direction
 * and every finite, non-zero point of that scan becomes NaN. This is not checked. */
int loamx_deskew_scans_dev(loamx_ctx* ctx, const double* d_xyz, size_t n_scans, const loamx_lidar_params* lidar,
                           const double* d_motion, double ref_fraction, double* d_xyz_out);
int loamx_deskew_scans_dev_f32(loamx_ctx* ctx, const float* d_xyz, size_t n_scans, const loamx_lidar_params* lidar,
                               const double* d_motion, double ref_fraction, float* d_xyz_out);
/* Debug / measurement (no reference counterpart, host arithmetic only, no context): the shape of the launch that
 * loamx_deskew_scans_dev[_f32] makes for n_scans scans of scan_lines x points_per_line points, from the function the launcher
 * itself calls. Each thread owns one column of one scan and walks a share of the scan lines.
 *   out[0] column blocks per scan (256 columns each; the last may be narrower)
 *   out[1] shares the lines of a scan are split into
 *   out[2] lines per share (the last share holds scan_lines - (out[1] - 1) * out[2] of them)
 *   out[3] lines a thread keeps in flight (the unroll of its loop; a share that is no multiple of it ends in a remainder)
 * An empty call (any of the three sizes 0) launches nothing: out[0..2] = 0. LOAMX_ERR_UNSUPPORTED for the sizes the de-skew
 * entry points refuse, LOAMX_ERR_BAD_PARAM for a null `out`. A test of "the remainder at shape X" asserts its shape from here. */
int loamx_deskew_launch_geometry(size_t n_scans, uint64_t scan_lines, uint64_t points_per_line, uint32_t out[4]);

/* ---- unordered clouds into scans (no reference counterpart: the reference demands an organised scan, common.h:104-113, and
 * leaves the projection to its users). Every entry point above starts from scan_lines x points_per_line points, row-major
 * [line][column]; sensor drivers and datasets deliver unordered x, y, z (with or without a ring number), with dropped returns
 * missing and, for dual-return sensors, two points per beam. These entry points put such a cloud into the grid on the device,
 * with a winner per cell that does not depend on how the threads are scheduled.
 *
 * A scan layout (H = scan_lines, W = points_per_line) holds two tables, computed once on the host in FP64 and kept on the device:
 *   column boundaries  u_k = (cos phi_k, sin phi_k), phi_k = azimuth_zero + sgn 2 pi (k - 1/2) / W, k = 0 .. W - 1; sgn = +1
 *                      counter-clockwise seen from +z, -1 when `clockwise` is set. With the defaults column c is centred on the
 *                      azimuth 2 pi c / W (the convention of the synthetic generator).
 *   line boundaries    t_0 .. t_H: the tangents of the elevations half way between neighbouring beams; the two outer ones lie
 *                      half the adjacent spacing beyond the outer beams. Beam elevations: `elevations`[H] (radians, strictly
 *                      ascending, line 0 the lowest beam) or, if NULL, linear from fov_bottom to fov_top. H == 1: {-inf, +inf}.
 * Per point p = (x, y, z) (float input is widened first; every product and sum is rounded on its own, no fused multiply-add):
 *   1. rho2 = x x + y y, r2 = rho2 + z z. INVALID (dropped): a non-finite coordinate, a non-finite r2, or !(rho2 >= 1e-100) —
 *      "no azimuth", which includes the all-zero point of a beam without a return.
 *   2. column: s_k = (sgn (u_k.x y - u_k.y x) >= 0); the column is the c with s_c true and s_(c + 1) mod W false (W == 1: 0).
 *   3. line, without rings: rho = sqrt(rho2), cnt = the number of l in 0 .. H with z >= t_l rho; cnt == 0 or H + 1: OUTSIDE the
 *      fan (dropped), else line cnt - 1. With rings (one uint16 per point): the line is ring, or ring_map[ring] if a map was
 *      given; a ring >= H, a ring beyond the map or a map entry 0xFFFF: OUTSIDE.
 *   4. winner of a cell among the points of one cloud: KEEP_FIRST the lowest input index (the voxel filter's rule);
 *      KEEP_NEAREST the smallest r2 (as doubles), on equal r2 the lowest index. The others are counted as collisions.
 *   5. the winner's three coordinates are copied bit for bit in the input's type; a cell without a winner is (+0, +0, +0) — for
 *      the extraction a beam without a return. src_idx[cell]: the winner's index within its cloud or 0xFFFFFFFF. stats per
 *      cloud: {filled, invalid, outside, collisions}; they add up to the cloud's point count.
 * The same bytes on every run, and for a cloud alone or inside any batch. */
enum { LOAMX_ORGANIZE_KEEP_FIRST = 0, LOAMX_ORGANIZE_KEEP_NEAREST = 1 };
typedef struct {
  double azimuth_zero;       /* 0.0: azimuth of the centre of column 0 (radians) */
  uint32_t clockwise;        /* 0 */
  uint32_t keep;             /* LOAMX_ORGANIZE_KEEP_FIRST */
  const double* elevations;  /* NULL: linear from fov_bottom to fov_top */
  double fov_bottom;         /* -15 degrees, in radians */
  double fov_top;            /* +15 degrees */
  const uint16_t* ring_map;  /* NULL: the ring number is the line. Entries: a line < scan_lines, or 0xFFFF (drop that ring) */
  size_t n_ring_map;
} loamx_organize_params;
void loamx_default_organize_params(loamx_organize_params* p);
typedef struct loamx_scan_layout loamx_scan_layout;
/* Copies everything it needs from *params (the arrays included). LOAMX_ERR_BAD_PARAM: a null argument, scan_lines or
 * points_per_line 0, an unknown `keep`, a non-finite value, elevations that do not ascend, fov_top <= fov_bottom with
 * scan_lines > 1, a boundary elevation outside (-pi/2, pi/2), a ring_map entry >= scan_lines other than 0xFFFF.
 * LOAMX_ERR_UNSUPPORTED: a shape the extraction refuses (points_per_line > 4096, more than 2^30 - 1 points). */
int loamx_scan_layout_create(loamx_ctx* ctx, const loamx_lidar_params* lidar, const loamx_organize_params* params,
                             loamx_scan_layout** out);
void loamx_scan_layout_destroy(loamx_ctx* ctx, loamx_scan_layout* layout);
/* The two tables exactly as the kernels use them (host copies of the uploaded bytes): col_dirs[W][2] = u_k, line_tans[H + 1].
 * Either may be NULL. A model of the rule above that reads them depends on nobody's cos or tan. */
int loamx_scan_layout_tables(const loamx_scan_layout* layout, double* col_dirs, double* line_tans);
/* n_clouds clouds stored back to back -> n_clouds scans.
 *   d_points       the points, point_stride scalars each (>= 3: x, y, z first; 4 is the x y z intensity of a KITTI file)
 *   d_rings        one uint16 per point, or NULL (lines by elevation)
 *   cloud_offsets  HOST array of n_clouds + 1 ascending point offsets (read before the call returns); a cloud may be empty,
 *                  its scan is then all zero
 *   d_scans        n_clouds x H W x 3 scalars of the input's type: what loamx_extract_features_batch_dev[_f32],
 *                  loamx_register_scan_sequence_dev[_f32] and loamx_deskew_scans_dev[_f32] take
 *   d_src_idx      n_clouds x H W uint32, or NULL;  d_stats: n_clouds x 4 uint32, or NULL
 * Every entry of the three outputs is written. Asynchronous on the context's stream, no synchronisation (the claim table
 * lives in the context's workspace and is reset by the call). LOAMX_ERR_BAD_PARAM: a null layout, d_points, cloud_offsets
 * or d_scans (n_clouds > 0), point_stride < 3, descending offsets; LOAMX_ERR_UNSUPPORTED: a cloud of more than 2^32 - 2
 * points. A refused call writes nothing. n_clouds == 0: LOAMX_OK. */
int loamx_organize_clouds_dev(loamx_ctx* ctx, const loamx_scan_layout* layout, const double* d_points, size_t point_stride,
                              const uint16_t* d_rings, const size_t* cloud_offsets, size_t n_clouds, double* d_scans,
                              uint32_t* d_src_idx, uint32_t* d_stats);
int loamx_organize_clouds_dev_f32(loamx_ctx* ctx, const loamx_scan_layout* layout, const float* d_points, size_t point_stride,
                                  const uint16_t* d_rings, const size_t* cloud_offsets, size_t n_clouds, float* d_scans,
                                  uint32_t* d_src_idx, uint32_t* d_stats);
/* One cloud of n_points points, host memory in, host memory out, synchronous; src_idx and stats may be NULL. */
int loamx_organize_cloud(loamx_ctx* ctx, const loamx_scan_layout* layout, const double* points, size_t point_stride,
                         const uint16_t* rings, size_t n_points, double* scan, uint32_t* src_idx, uint32_t* stats);
int loamx_organize_cloud_f32(loamx_ctx* ctx, const loamx_scan_layout* layout, const float* points, size_t point_stride,
                             const uint16_t* rings, size_t n_points, float* scan, uint32_t* src_idx, uint32_t* stats);

/* ---- place recognition (no reference counterpart: SURVEY 2 negatives). A mapper notices that it has been somewhere before by
 * comparing a descriptor of the current scan with the descriptors of earlier scans: here the Scan Context form, a polar grid of
 * maximum heights with a rotation-invariant ring key as pre-filter, compared under every column shift; the best shift is a yaw
 * guess for the registration that makes the loop edge. Everything below is integer or individually rounded FP64, the device
 * uses no libm beyond sqrt and floor, and nothing depends on thread scheduling: a model can be compared by equality of bytes.
 *
 * Parameters: R = n_rings, S = n_sectors, L = max_range, z_offset, z_scale. ring_scale = R / L is formed once on the host in
 * double. The S sector boundaries are those of a scan layout of S columns with azimuth_zero 0, counter-clockwise: sector c is
 * centred on the azimuth 2 pi c / S. The table is computed on the host, kept on the device, and handed out byte for byte.
 * Per point p = (x, y, z) in the sensor frame (float input is widened first; every product and sum is rounded on its own):
 *   1. validity as in "unordered clouds into scans", step 1: dropped if a coordinate or r2 is not finite or !(rho2 >= 1e-100),
 *      which includes the all-zero cell of an organised scan.
 *   2. ring: rho = sqrt(rho2), f = rho ring_scale; dropped if !(f < R), else ring = floor(f).
 *   3. sector: the column of "unordered clouds into scans", step 2, on the table of S boundaries.
 *   4. code: h = floor((z + z_offset) z_scale) clamped to [0, 65534], code = h + 1 (1 .. 65535; 0 means no point).
 * Descriptor: R x S uint16, row-major [ring][sector], the maximum code of each cell; an empty cloud gives all zeros.
 *   ring key     R x uint32: the sum of each ring's codes.
 *   column norm  S x uint64: the sum of the squared codes of each sector.
 * Key distance of a query and an entry: sum_r (key_q[r] - key_e[r])^2, exact in uint64 (< 2^63).
 * Distance under shift s in [0, S): for sector j, column q[:, j] against e[:, (j + s) mod S]:
 *   dot_j  exact in uint64. The pair of columns counts when both norms are non-zero; m = the number of such pairs.
 *   c_j    = (double) dot_j / sqrt((double) nq_j (double) ne_j'), each operation rounded on its own. (The product comes
 *            before the root so that a column against itself has c_j = 1.0 exactly: sqrt(fl(n n)) = n for an integer
 *            n < 2^53, while sqrt(n) sqrt(n) misses n for most n. A descriptor against a rolled copy has distance 0.0.)
 *   k_j    = min((uint64) floor(c_j 2^30), 2^30)
 *   score  = sum_j k_j;  dist = 1.0 - (double) score / ((double) m 2^30), or 1.0 when m == 0
 * The distance of the pair is the smallest dist over s; on a tie the lowest s. s is the number of sectors the query sensor is
 * turned counter-clockwise (seen from +z) relative to the entry's: a rotation about z by s 2 pi / S is the entry_T_query guess.
 * Search of one query with K = num_candidates and id_end: among the entries with id < id_end the K smallest by (key distance,
 * id) — exhaustively — get their shift distance over all S shifts; the K records come back ascending by (distance, id), the
 * slots beyond the number of eligible entries as {0xFFFFFFFF, 0, 2^64 - 1, 2.0}. */
typedef struct {
  uint32_t n_rings;   /* 20 */
  uint32_t n_sectors; /* 60 */
  double max_range;   /* 80.0 */
  double z_offset;    /* 2.0: sensor height above ground; makes heights positive */
  double z_scale;     /* 64.0: codes per metre; a power of two keeps the product exact */
} loamx_place_params;
void loamx_default_place_params(loamx_place_params* p);
typedef struct {
  uint32_t id;       /* the entry, or 0xFFFFFFFF */
  uint32_t shift;    /* sectors the query is turned counter-clockwise relative to the entry */
  uint64_t key_dist; /* squared ring-key distance */
  double distance;   /* 0 .. 1; 2.0 without an entry */
} loamx_place_match;
typedef struct loamx_place_db loamx_place_db;
/* The database owns the parameters, the sector table and the stored entries (descriptor, ring key, column norms per entry; ids
 * are consecutive from 0, at most 2^24). LOAMX_ERR_BAD_PARAM: a null argument, n_rings or n_sectors 0, a non-finite or
 * non-positive max_range or z_scale, a non-finite z_offset. LOAMX_ERR_UNSUPPORTED: n_rings > 64, n_sectors < 3 (the column has
 * no unique answer at two boundaries or fewer) or > 360. */
int loamx_place_db_create(loamx_ctx* ctx, const loamx_place_params* params, loamx_place_db** out);
void loamx_place_db_destroy(loamx_ctx* ctx, loamx_place_db* db);
/* dirs[S][2]: the sector table exactly as the kernels use it (a host copy of the uploaded bytes) */
int loamx_place_db_sector_dirs(const loamx_place_db* db, double* dirs);
int loamx_place_db_size(const loamx_place_db* db, size_t* n_entries);
/* n_clouds clouds stored back to back -> n_clouds descriptors of R S uint16 in d_desc; d_points, point_stride and cloud_offsets
 * (HOST, n_clouds + 1) as for loamx_organize_clouds_dev: an organised scan is a cloud of H W points. Every entry of d_desc is
 * written. Asynchronous on the context's stream; no synchronisation unless the workspace has to grow. The database is not
 * changed. LOAMX_ERR_BAD_PARAM: a null db, d_points (with points), cloud_offsets or d_desc, point_stride < 3, descending
 * offsets; LOAMX_ERR_UNSUPPORTED: a cloud of more than 2^32 - 2 points. A refused call writes nothing. n_clouds == 0: LOAMX_OK. */
int loamx_place_descriptors_dev(loamx_ctx* ctx, const loamx_place_db* db, const double* d_points, size_t point_stride,
                                const size_t* cloud_offsets, size_t n_clouds, uint16_t* d_desc);
int loamx_place_descriptors_dev_f32(loamx_ctx* ctx, const loamx_place_db* db, const float* d_points, size_t point_stride,
                                    const size_t* cloud_offsets, size_t n_clouds, uint16_t* d_desc);
/* Appends n descriptors (device) as the entries *first_id .. *first_id + n - 1 (first_id may be NULL) and derives their keys
 * and norms. Asynchronous unless the database has to grow. LOAMX_ERR_UNSUPPORTED beyond 2^24 entries; a refused call leaves
 * the database as it was. n == 0: LOAMX_OK. */
int loamx_place_db_add_dev(loamx_ctx* ctx, loamx_place_db* db, const uint16_t* d_desc, size_t n, uint32_t* first_id);
/* Host read-back of the entries first .. first + count - 1: desc[count][R S], keys[count][R], norms[count][S]; any may be NULL.
 * Synchronises. LOAMX_ERR_BAD_PARAM beyond the database's size. */
int loamx_place_db_read(loamx_ctx* ctx, const loamx_place_db* db, size_t first, size_t count, uint16_t* desc, uint32_t* keys,
                        uint64_t* norms);
/* n_queries descriptors (device) -> n_queries x num_candidates records in d_out, every one written. id_end: HOST array of
 * n_queries values (read before the call returns), or NULL: every entry. Asynchronous unless the workspace has to grow.
 * LOAMX_ERR_BAD_PARAM: a null db, d_query_desc or d_out, num_candidates outside 1 .. 64. n_queries == 0: LOAMX_OK. */
int loamx_place_search_dev(loamx_ctx* ctx, const loamx_place_db* db, const uint16_t* d_query_desc, size_t n_queries,
                           const uint32_t* id_end, uint32_t num_candidates, loamx_place_match* d_out);
/* Host memory in, host memory out, synchronous: one cloud -> its descriptor; n_queries descriptors -> their records. */
int loamx_place_descriptor(loamx_ctx* ctx, const loamx_place_db* db, const double* points, size_t point_stride, size_t n_points,
                           uint16_t* desc);
int loamx_place_descriptor_f32(loamx_ctx* ctx, const loamx_place_db* db, const float* points, size_t point_stride,
                               size_t n_points, uint16_t* desc);
int loamx_place_search(loamx_ctx* ctx, const loamx_place_db* db, const uint16_t* query_desc, size_t n_queries,
                       const uint32_t* id_end, uint32_t num_candidates, loamx_place_match* out);

/* ---- pose graph (no reference counterpart). The consumer of everything above: odometry edges from a scan sequence, loop edges
 * from place recognition and a registration, each weighted by its loamx_reg_information matrix, corrected together by a sparse
 * SE(3) least-squares solve: Levenberg-Marquardt over block-Jacobi preconditioned conjugate gradients. Poses, edges and the result
 * stay on the device; a solve reads nothing back. Everything is FP64 rounded operation by operation, the device uses no libm
 * beyond sqrt and no floating-point atomics, and nothing depends on thread scheduling: the same bytes on every run, and a
 * host build of the same arithmetic (loam_amd/csrc/posegraph_math.h) can be compared by equality of bytes.
 *
 * Poses are world_T_i as pose7, composed with the arithmetic of Pose3d::compose; inv(T) = (conj(q), -(conj(q) rotating t)).
 * Edge: Z = a_T_b measures pose b in the frame of pose a (a in the target role, b in the source role): pair p of a sequence is
 *   the edge (p, p + 1, results[p].pose, info[p].information), a loop edge is (old, new, old_T_new, its information).
 *   information is in the basis of loamx_reg_information: left perturbation Z <- (Exp(omega), t) o Z, rotation first; only its
 *   upper triangle is read, and it is mirrored.
 * Error of an edge:  zhat = inv(T_a) o T_b;  q_D = q_zhat (x) conj(q_Z);  t_D = t_zhat - q_D rotating t_Z;
 *   e = [2 sgn(w_D) (x_D, y_D, z_D), t_D] with sgn(0) = +1 (to first order the (omega, t) of the information's basis; no atan2);
 *   chi2 = e . (Omega e), Omega e row by row. A measurement composed from the poses by the same arithmetic has e = 0 exactly.
 * Variables: a right perturbation delta_i = (omega_i, tau_i) of every pose that is not fixed, with the retraction
 *   T_i <- T_i o (normalise([omega_i / 2, 1]), tau_i).  A = de/d delta_a and B = de/d delta_b at delta = 0 are closed forms
 *   (posegraph_math.h: pgo_jacobians), row-major 6 x 6, columns omega then tau.
 * Huber (huber_delta > 0 and chi2 > delta^2): the edge's blocks and gradients are scaled by w = delta / chi and its cost is
 *   2 delta chi - delta^2; otherwise w = 1 and the cost is chi2. The cost of a graph is the sum of its edges' costs.
 * Normal equations: per edge H_aa = w A^T Omega A, H_ab = w A^T Omega B, H_bb = w B^T Omega B, g_a = w A^T Omega e,
 *   g_b = w B^T Omega e; per pose the diagonal block and gradient are the sums over its incident (edge, side) entries in
 *   ascending (edge, side) order (side 0: the pose is the edge's a). Fixed poses have delta = 0 and leave the system.
 * Levenberg-Marquardt: the diagonal entry D_kk becomes D_kk + lambda max(D_kk, 1e-6) (the floor keeps a pose whose edges carry
 *   no information solvable); lambda starts at initial_lambda. An iteration solves for delta, forms the candidate poses and
 *   their cost c1 and then, with c0 the cost before and m = max |delta_k| over all poses:
 *     m <= step_tolerance                          STEP_CONVERGED, the poses stay as they were (checked first);
 *     c1 < c0                                      accepted: the candidate becomes the poses, lambda <- max(lambda / 10, 1e-12),
 *                                                  and COST_CONVERGED if c0 - c1 <= cost_tolerance c0;
 *     otherwise                                    rejected: lambda <- 10 lambda, LAMBDA_OVERFLOW if lambda > 1e12;
 *     then MAX_ITERATIONS once max_iterations iterations have run.
 * Inner solve: PCG from x = 0 on (H + damping) x = -g, preconditioned by the Cholesky inverses of the damped 6 x 6 diagonal
 *   blocks (a block whose Cholesky meets a non-positive pivot takes its pose out of the system for that iteration). It stops
 *   at r.z <= pcg_tolerance^2 r0.z0, after min(max_pcg_iterations, 6 n_poses) iterations (conjugate gradients end within as
 *   many steps as there are unknowns in exact arithmetic), or at p.q <= 0, where it keeps x. A truncated solve is still a
 *   descent step.
 * Sums that cross threads (the cost, r.z, p.q, max |delta|): per edge or per pose in index order, fixed chunks of 256 reduced by
 *   the tree of posegraph_math.h (strides 128 ... 1), the chunks added in ascending order.
 * Edge indices are checked before anything is indexed with them: an edge with a == b, a >= n_poses or b >= n_poses is counted
 *   and never followed. */
enum {
  LOAMX_PGO_COST_CONVERGED = 0,
  LOAMX_PGO_STEP_CONVERGED = 1,
  LOAMX_PGO_MAX_ITERATIONS = 2,
  LOAMX_PGO_LAMBDA_OVERFLOW = 3,
  LOAMX_PGO_NOTHING_TO_DO = 4, /* no poses, no edges, or no pose that is not fixed */
  LOAMX_PGO_BAD_INPUT = 5      /* some edge is invalid: n_bad_edges of them; the poses are untouched */
};
typedef struct {
  uint32_t a, b;
  double a_T_b[7];
  double information[36];
} loamx_pgo_edge; /* 352 bytes */
typedef struct {
  uint32_t max_iterations;     /* 20 */
  uint32_t max_pcg_iterations; /* 500 */
  double pcg_tolerance;        /* 1e-8 */
  double initial_lambda;       /* 1e-4 */
  double cost_tolerance;       /* 1e-9 */
  double step_tolerance;       /* 1e-10 */
  double huber_delta;          /* 0: off */
} loamx_pgo_params;
void loamx_pgo_default_params(loamx_pgo_params* p);
typedef struct {
  double initial_cost, final_cost;
  double lambda;               /* after the last iteration */
  double max_update;           /* max |delta_k| of the last iteration */
  uint32_t iterations;         /* LM iterations run */
  uint32_t accepted;           /* of those, accepted */
  uint32_t pcg_iterations;     /* total over the solve */
  uint32_t termination;        /* LOAMX_PGO_* */
  uint32_t n_bad_edges;
  uint32_t reserved;           /* 0 */
} loamx_pgo_summary; /* 56 bytes */
/* one edge as the solver's linearisation kernel sees it */
typedef struct {
  double e[6];
  double chi2;
  double weight;
  double A[36], B[36];
} loamx_pgo_linearization; /* 640 bytes */
/* d_poses: n_poses x 7, in and out; d_fixed: n_poses bytes, non-zero = fixed, or NULL = pose 0 only; d_summary: one record, or
 * NULL. Asynchronous on the context's stream; no synchronisation unless the workspace has to grow. With an invalid edge the
 * poses are left untouched and the summary says LOAMX_PGO_BAD_INPUT with n_bad_edges. n_poses == 0 or n_edges == 0:
 * LOAMX_PGO_NOTHING_TO_DO. LOAMX_ERR_BAD_PARAM: a null ctx, params, d_poses or d_edges (with poses / edges), a non-finite
 * parameter, a negative tolerance or huber_delta, initial_lambda <= 0, max_iterations == 0; LOAMX_ERR_UNSUPPORTED: 2^31 poses
 * or edges or more. The device form does not look at the values of the poses and edges. */
int loamx_pose_graph_optimize_dev(loamx_ctx* ctx, double* d_poses, size_t n_poses, const uint8_t* d_fixed, const loamx_pgo_edge* d_edges,
                                  size_t n_edges, const loamx_pgo_params* params, loamx_pgo_summary* d_summary);
/* Host memory in, host memory out, synchronous. Further LOAMX_ERR_BAD_PARAM: a null summary, a non-finite pose, measurement or
 * information entry, an invalid edge, no fixed pose. n_poses == 0 or n_edges == 0: LOAMX_OK, LOAMX_PGO_NOTHING_TO_DO, the poses
 * unchanged. A refused call writes nothing. */
int loamx_pose_graph_optimize(loamx_ctx* ctx, double* poses, size_t n_poses, const uint8_t* fixed, const loamx_pgo_edge* edges,
                              size_t n_edges, const loamx_pgo_params* params, loamx_pgo_summary* summary);
/* Host form: e, chi2, weight, A, B of every edge at the given poses, by the solver's own linearisation kernel read out instead
 * of consumed (what loamx_associate is to the registration). huber_delta as in the parameters (0: off). Refusals as above. */
int loamx_pose_graph_linearize(loamx_ctx* ctx, const double* poses, size_t n_poses, const loamx_pgo_edge* edges, size_t n_edges,
                               double huber_delta, loamx_pgo_linearization* out);
/* The odometry edges of a sequence: pair p becomes d_edges[p] = (first_id + p, first_id + p + 1, d_results[p].pose,
 * d_info[p].information), so that a drive goes sequence -> edges -> optimise without leaving the device. Asynchronous. */
int loamx_pose_graph_edges_from_results_dev(loamx_ctx* ctx, const loamx_reg_result* d_results, const loamx_reg_information* d_info,
                                            size_t n_pairs, uint32_t first_id, loamx_pgo_edge* d_edges);

/* ---- cloud map (no reference counterpart). What a mapper exists to produce: all points of all scans at their poses, thinned on
 * a voxel grid to ONE CENTROID PER VOXEL (PCL's VoxelGrid), held on the device, and rebuilt from corrected poses in one call
 * after a pose-graph solve without the poses leaving the device. The sums are taken in integers, so every schedule, every split
 * over workgroups and every partial combine gives the same bytes; a numpy model is compared by equality (tests/cloudmap_common.py).
 * FP64 throughout, every product, quotient, sum and difference rounded on its own; float input is widened first.
 *
 * Per point p of cloud c (loam_amd/csrc/cloudmap_math.h):
 *   validity   dropped and counted `invalid` if a coordinate or r2 = x x + y y + z z is not finite; dropped and counted `range`
 *              if !(r2 >= min_range^2) || !(r2 <= max_range^2) (the squares are formed once on the host; min_range > 0 removes
 *              the all-zero cells of an organised scan).
 *   transform  p' = pose_c.act(p) (Pose3d::act; the quaternion is used as given), pose_c read from DEVICE memory: n_clouds x 7
 *              doubles as loamx_compose_trajectory_dev and loamx_pose_graph_optimize_dev leave them. No pose array: p' = p.
 *   voxel      per axis t = p'[a] / leaf (an IEEE division), v = floor(t); |v| < 2^20 as in "map upkeep", otherwise the point is
 *              dropped and counted `outside`; key as there.
 *   offset     frac = t - v (one rounded subtraction: t = -1e-20 gives exactly 1.0), u = min((uint64) floor(frac 2^32), 2^32 - 1).
 *   voxel sums sum[a] += u[a] (uint64), count += 1 (uint32), first = min(first, g) with g the point's running index: the
 *              points offered to the map before this call plus its index in the call's array counted from cloud_offsets[0].
 *              Dropped points keep their index. At most 2^32 - 2 points may be offered between two clears, so neither a count
 *              nor a sum can wrap.
 *   centroid   c[a] = ((double) v + ((double) sum[a] / (double) count) / 4294967296.0) leaf.
 * Voxel order. The voxels of a map are listed by ascending `first`: in order of first appearance across all calls since the
 *   last clear. The order is kept as data (a list of table slots, appended to by every add); it is not obtained by sorting and
 *   does not depend on which slot a voxel won.
 * Storage. A table of 2^k >= 2 max_voxels slots (key, first, three sums and count: 40 B each), the list of max_voxels words, a
 *   few counters and the scratch of one round of launches (21 MB), all allocated at create and never grown: add, emit and
 *   clear never synchronise.
 * Overflow. `overflow` counts the points whose probe gave up after 2^k slots (they went into no voxel) plus ONE per new voxel
 *   that did not fit the list, for the point that opened it (such a voxel keeps taking sums, its points count as used, and it
 *   is never emitted). No launch spins or writes out of bounds.
 *   FROM THE FIRST OVERFLOW UNTIL THE NEXT CLEAR the map promises only that every call returns and that the stats say so:
 *   which voxels it lists, and in which order, is then unspecified. */
typedef struct {
  double leaf;      /* 0.2 */
  double min_range; /* 0.5 */
  double max_range; /* 120.0 */
} loamx_cloud_map_params;
typedef struct {
  uint64_t voxels;         /* voxels in the list */
  uint64_t points_offered; /* since the last clear, dropped ones included */
  uint64_t points_used;    /* points that went into a voxel's sums */
  uint64_t invalid, range, outside;
  uint64_t overflow;
} loamx_cloud_map_stats;
/* A map belongs to the context it was created on: every other entry point refuses it on another context (LOAMX_ERR_BAD_PARAM).
 * The scratch of an add and of an emit lives in the map (so emit, which leaves the voxels alone, still writes to the handle's
 * device memory), and the context's mutex and stream put its uses in order: calls from several threads are safe, and two emits
 * or an add and an emit never overlap on the device. */
typedef struct loamx_cloud_map loamx_cloud_map;
void loamx_default_cloud_map_params(loamx_cloud_map_params* p);
/* LOAMX_ERR_BAD_PARAM: a null argument, leaf not finite or <= 0, a negative or non-finite min_range, max_range < min_range (or
 * NaN), max_voxels == 0; LOAMX_ERR_UNSUPPORTED: max_voxels > 2^30. */
int loamx_cloud_map_create(loamx_ctx* ctx, const loamx_cloud_map_params* params, size_t max_voxels, loamx_cloud_map** out);
void loamx_cloud_map_destroy(loamx_ctx* ctx, loamx_cloud_map* map);
/* an empty map again, running index 0. Asynchronous on the context's stream. */
int loamx_cloud_map_clear(loamx_ctx* ctx, loamx_cloud_map* map);
/* n_clouds device-resident clouds back to back: cloud c holds the points cloud_offsets[c] .. cloud_offsets[c + 1] - 1 of d_points,
 * point_stride scalars apart (the conventions of loamx_organize_clouds_dev: cloud_offsets is a HOST array of n_clouds + 1
 * entries, an organised scan is a cloud of H W points, a cloud may be empty). d_poses: DEVICE, n_clouds x 7, or NULL = no
 * transform. Asynchronous, no host round trip: it composes behind loamx_pose_graph_optimize_dev without a synchronise.
 * LOAMX_ERR_BAD_PARAM: a null map, cloud_offsets or d_points (with points), point_stride < 3, descending offsets;
 * LOAMX_ERR_UNSUPPORTED: more than 2^32 - 2 points offered since the last clear with this call's, a point_stride beyond 32 bits.
 * A refused call changes nothing. n_clouds == 0: LOAMX_OK. */
int loamx_cloud_map_add_clouds_dev(loamx_ctx* ctx, loamx_cloud_map* map, const double* d_points, size_t point_stride,
                                   const size_t* cloud_offsets, size_t n_clouds, const double* d_poses);
int loamx_cloud_map_add_clouds_dev_f32(loamx_ctx* ctx, loamx_cloud_map* map, const float* d_points, size_t point_stride,
                                       const size_t* cloud_offsets, size_t n_clouds, const double* d_poses);
/* The centroids of the voxels with count >= min_points, in list order, to DEVICE memory: d_xyz_out (capacity x 3), d_count_out and
 * d_first_out (capacity each; either may be NULL). At most `capacity` are written; *d_n_out is the number that qualify even
 * when it exceeds capacity. Every entry below min(n, capacity) of each non-null output is written and nothing beyond. The map
 * is not changed. Asynchronous. LOAMX_ERR_BAD_PARAM: a null map or d_n_out, a null d_xyz_out with capacity > 0. */
int loamx_cloud_map_emit_dev(loamx_ctx* ctx, const loamx_cloud_map* map, uint32_t min_points, double* d_xyz_out, uint32_t* d_count_out,
                             uint32_t* d_first_out, size_t capacity, uint32_t* d_n_out);
/* synchronises */
int loamx_cloud_map_stats_read(loamx_ctx* ctx, const loamx_cloud_map* map, loamx_cloud_map_stats* out);
/* Measurement read-out: the claims since the last clear, that is, how often the accumulate kernel began a probe (one 64-bit
 * CAS, more when the probe walks) followed by its five atomics: once per used point in the plain form, once per run of a
 * wavefront with run combining. Changes nothing; synchronises. */
int loamx_cloud_map_claims_read(loamx_ctx* ctx, const loamx_cloud_map* map, uint64_t* claims);
/* host forms, synchronous: one cloud in host memory with a HOST pose (NULL = no transform); the emit to host arrays, *n_out the
 * number that qualify */
int loamx_cloud_map_add_cloud(loamx_ctx* ctx, loamx_cloud_map* map, const double* points, size_t point_stride, size_t n_points,
                              const double pose[7]);
int loamx_cloud_map_add_cloud_f32(loamx_ctx* ctx, loamx_cloud_map* map, const float* points, size_t point_stride, size_t n_points,
                                  const double pose[7]);
int loamx_cloud_map_emit(loamx_ctx* ctx, const loamx_cloud_map* map, uint32_t min_points, double* xyz_out, uint32_t* count_out,
                         uint32_t* first_out, size_t capacity, size_t* n_out);

/* ---- scan segmentation (no reference counterpart; the range-image pass LeGO-LOAM and LIO-SAM put in front of the extraction).
 * Labels the ground of an organised scan, clusters the rest by connected components under an angle criterion, and tells the
 * components too small to be a surface (leaves, wires, rain, the edges of moving objects) from the others. Everything is integer
 * or individually rounded FP64, roots are minima and counts are integer sums: two runs give the same bytes, a scan alone or inside
 * a batch gives the same bytes, and a numpy model is compared by equality on every cell (tests/segment_common.py).
 *
 * The rule (loam_amd/csrc/segment_math.h). Every product, sum and difference is one FP64 operation rounded on its own, in the
 * order written; float input is widened first. A scan is scan_lines (H) x points_per_line (W) cells, row-major, i = l W + c.
 *   valid      a cell is valid iff its three coordinates are finite and sqrt((x x + y y) + z z), the extraction's range, is not
 *              < min_range and not > max_range (the extraction's own comparison). (0, 0, 0) and NaN cells are invalid; they are
 *              never refused.
 *   ground     G = ground_lines, or H when that is 0 or larger than H. For every column c and every l with l + 1 < G the cells
 *              (l, c), (l + 1, c) are a ground pair iff both are valid and dz dz <= tg2 (dx dx + dy dy), d = p(l + 1, c) - p(l, c),
 *              tg2 = tan(ground_angle)^2. A cell is ground iff it belongs to at least one ground pair.
 *   nodes      the valid cells that are not ground. Candidate edges per cell: right, (l, c) - (l, (c + 1) mod W) (none when
 *              W == 1; when W == 2 the same pair appears from both cells); up, (l, c) - (l + 1, c) (lines do not wrap).
 *   connected  two nodes a, b joined by a candidate edge are connected iff t t < (c2 m) e2, where r2 = (x x + y y) + z z per point,
 *              m = max(r2a, r2b), dot = (ax bx + ay by) + az bz, e = b - a, e2 = (ex ex + ey ey) + ez ez, t = m - dot and
 *              c2 = cos(segment_angle)^2: the angle at the farther point between the ray to the sensor and the chord to the nearer
 *              point exceeds segment_angle (LeGO-LOAM's test without atan2, sqrt or the sensor's angular resolution). The
 *              expression is symmetric in a and b to the bit: the graph is undirected.
 *   components the connected components of that graph. Label = the smallest linear index (the root); size = the number of cells;
 *              line span = max line - min line + 1. Accepted iff size >= min_cluster_points, or size >= min_tall_cluster_points
 *              and span >= min_tall_cluster_lines. Cells of accepted components are class cluster, the others class outlier.
 * tg2 and c2 are formed once per call on the host (FP64, libm); loamx_segment_constants returns the same two numbers. */
typedef struct {
  uint64_t ground_lines;            /* 0 (all lines) */
  double ground_angle;              /* 10 degrees, in radians */
  double segment_angle;             /* 60 degrees, in radians */
  uint64_t min_cluster_points;      /* 30 */
  uint64_t min_tall_cluster_points; /* 5 */
  uint64_t min_tall_cluster_lines;  /* 3 */
  uint32_t drop_outliers;           /* 1 */
  uint32_t drop_ground;             /* 0 */
} loamx_segment_params;
enum { LOAMX_SEGMENT_INVALID = 0, LOAMX_SEGMENT_GROUND = 1, LOAMX_SEGMENT_CLUSTER = 2, LOAMX_SEGMENT_OUTLIER = 3 };
#define LOAMX_SEGMENT_NO_LABEL 0xFFFFFFFFu
typedef struct {
  uint32_t root, size, line_min, line_max;
} loamx_segment_cluster;
void loamx_default_segment_params(loamx_segment_params* p);
/* out = {tg2, c2} exactly as the launcher computes them. Needs no context. LOAMX_ERR_BAD_PARAM as listed below for the angles. */
int loamx_segment_constants(const loamx_segment_params* params, double out[2]);
/* n_scans device-resident scans back to back (n_scans x H x W x 3 scalars). Outputs per scan, back to back over the batch, each
 * pointer may be NULL:
 *   d_classes   uint8 per cell: LOAMX_SEGMENT_INVALID / _GROUND / _CLUSTER / _OUTLIER
 *   d_labels    uint32 per cell: the root for cluster and outlier cells, LOAMX_SEGMENT_NO_LABEL otherwise
 *   d_sizes     uint32 per cell: the size of the cell's component for cluster and outlier cells, 0 otherwise
 *   d_filtered  a scan of the input's scalar type: invalid cells, outlier cells under drop_outliers and ground cells under
 *               drop_ground become (+0, +0, +0); every other cell's three scalars are copied bit for bit. May be exactly d_scans
 *               (in place); any other overlap is the caller's error.
 *   d_clusters  the accepted components in ascending root order, max_clusters records per scan of which the first
 *               min(accepted, max_clusters) are written (an ordered compaction: never a sort, never arrival order)
 *   d_stats     uint32[8] per scan: {invalid, ground, cluster cells, outlier cells, accepted components, rejected components,
 *               largest component size, cluster records written}
 * Asynchronous on the context's stream; synchronises only when the workspace has to grow. LOAMX_ERR_BAD_PARAM: a null params or
 * lidar, scan_lines or points_per_line 0, a non-finite angle, ground_angle outside [0, pi/2), segment_angle outside (0, pi/2), a
 * max_range whose fourth power is not finite, a null d_scans with n_scans > 0. LOAMX_ERR_UNSUPPORTED: points_per_line > 4096 or
 * more than 2^30 - 1 cells (the extraction's limits), more than 65535 scans. A refused call writes nothing. n_scans == 0: LOAMX_OK.
 *
 * Kernels (loam_amd/csrc/segment_kernels.hip): classes and ground per cell; the components of each 16 x 256 tile by a union-find in
 * LDS; the connected edges that cross a tile border (and the seam edges) through a union on global parents; a separate launch
 * flattens. Context option NO_SEGMENT_TILES: every parent starts as its own index and ALL connected edges go through the global
 * union — the same bytes. */
int loamx_segment_scans_dev(loamx_ctx* ctx, const double* d_scans, size_t n_scans, const loamx_lidar_params* lidar,
                            const loamx_segment_params* params, uint8_t* d_classes, uint32_t* d_labels, uint32_t* d_sizes,
                            double* d_filtered, loamx_segment_cluster* d_clusters, size_t max_clusters, uint32_t* d_stats);
int loamx_segment_scans_dev_f32(loamx_ctx* ctx, const float* d_scans, size_t n_scans, const loamx_lidar_params* lidar,
                                const loamx_segment_params* params, uint8_t* d_classes, uint32_t* d_labels, uint32_t* d_sizes,
                                float* d_filtered, loamx_segment_cluster* d_clusters, size_t max_clusters, uint32_t* d_stats);
/* one scan, host memory in, host memory out, synchronous; further LOAMX_ERR_BAD_PARAM: a null scan */
int loamx_segment_scan(loamx_ctx* ctx, const double* scan, const loamx_lidar_params* lidar, const loamx_segment_params* params,
                       uint8_t* classes, uint32_t* labels, uint32_t* sizes, double* filtered, loamx_segment_cluster* clusters,
                       size_t max_clusters, uint32_t* stats);
int loamx_segment_scan_f32(loamx_ctx* ctx, const float* scan, const loamx_lidar_params* lidar, const loamx_segment_params* params,
                           uint8_t* classes, uint32_t* labels, uint32_t* sizes, float* filtered, loamx_segment_cluster* clusters,
                           size_t max_clusters, uint32_t* stats);
/* The last segmentation call of the context: out = {tile lines, tile columns, tiles per scan, connected edges handed to the global
 * union counted per cell and direction over the whole call, form: 1 tiles, 0 global-only}. An edge is handed over in the tile form
 * iff it is an up edge from the last line of a tile, a right edge from the last column of a tile, or a right edge from column
 * W - 1 (the seam, even where one tile holds both ends); in the global-only form always. Synchronises. LOAMX_ERR_BAD_PARAM before
 * any segmentation call. Never part of a result. */
int loamx_ctx_last_segment_census(loamx_ctx* ctx, uint64_t out[5]);

/* ---- map cleaning (no reference counterpart; the visibility check of Removert and of OctoMap-style free-space carving). A cloud
 * map keeps everything the sensor ever hit, a passing car included. For every pair of a map point and a scan this asks: did the
 * beam that looked towards the point stop at it, stop before it, or pass through it? A point that many scans saw through and few
 * confirmed belonged to a moving object. The votes are integer counts, so every schedule and both forms of the kernel give the
 * same bytes, and a numpy model is compared by equality (tests/visibility_common.py).
 *
 * The rule (loam_amd/csrc/visibility_math.h). FP64 throughout, float scans are widened first; every product, sum and difference
 * is one operation rounded on its own, in the order written; the only libm call is sqrt. The host forms
 * min2 = min_range min_range and max2 = max_range max_range once per call.
 * Per map point m (world frame) and scan s with pose world_T_s = (q, t) read from DEVICE memory (n_scans x 7 doubles):
 *   1 sensor frame  d = m - t component-wise; p = quat_rotate(conj(q), d) with conj(q) = (-qx, -qy, -qz, qw), quat_rotate the
 *                   rotation of Pose3d::act (v + qw (2 u x v) + u x (2 u x v)); the quaternion is used as given.
 *   2 has a place   the validity test of "unordered clouds into scans" must hold for p (finite, rho2 = x x + y y >= 1e-100),
 *                   with r2 = rho2 + z z; otherwise the verdict is NONE. If !(r2 >= min2) || !(r2 <= max2): NONE.
 *   3 cell          the organiser's cell of p WITHOUT ring numbers: the column by the layout's column boundaries, the line by the
 *                   elevation; the layout's ring map and keep rule are ignored. Outside the elevation fan: NONE. Otherwise
 *                   l = cell / W, c = cell % W.
 *   4 bounds        dist = sqrt(r2); tol = margin + margin_rel dist; lo = dist - tol, taken as 0 when negative; hi = dist + tol;
 *                   lo2 = lo lo; hi2 = hi hi.
 *   5 window        the cells (l + dl, (c + dc) mod W) for |dl| <= window_lines with 0 <= l + dl < H and |dc| <= window_cols: lines
 *                   do not wrap, columns do. (A cell met twice when 2 window_cols + 1 > W changes nothing: the reductions below
 *                   are `any` and `all`.) A cell is USABLE iff its three coordinates are finite and r2c = (x x + y y) + z z
 *                   satisfies r2c >= min2: NaN cells never are, (0, 0, 0) cells are not while min_range > 0. A usable cell AGREES iff r2c >= lo2 && r2c <= hi2
 *                   and is BEYOND iff r2c > hi2.
 *   6 verdict       EMPTY: no usable cell. AGREE: some usable cell agrees. THROUGH: otherwise, if every usable cell is beyond.
 *                   OCCLUDED: otherwise.
 *   7 votes         each field of the point's loamx_visibility_tally counts the scans with that verdict; NONE counts nowhere.
 * A point is DYNAMIC iff through >= min_through && (double) through >= through_ratio (double) agree (one rounded product).
 * The default window of one line and one column each way is what makes the test usable on ground seen at a grazing angle: the
 * beam through the point's own cell hits the ground metres further on, but the line below returns from in front of the point,
 * THROUGH needs every usable cell beyond, and the verdict is OCCLUDED. */
typedef struct {
  double min_range;      /* 1.0 */
  double max_range;      /* 80.0 */
  double margin;         /* 0.3 */
  double margin_rel;     /* 0.01 */
  uint32_t window_lines; /* 1; at most 3 */
  uint32_t window_cols;  /* 1; at most 3 */
  uint32_t min_through;  /* 2 */
  double through_ratio;  /* 1.0 */
} loamx_visibility_params;
typedef struct {
  uint32_t through, agree, occluded, empty;
} loamx_visibility_tally;
typedef struct {
  uint32_t form;           /* 1: the window reads squared ranges a first launch wrote; 0: it reads the scans' points (NO_VISIBILITY_RANGES) */
  uint32_t scan_chunks;    /* workgroup rows the scans were dealt over */
  uint64_t in_range_pairs; /* (point, scan) pairs that passed step 2 */
  uint64_t projected_pairs; /* ... and step 3: the sum of all four fields over all points that this call added */
} loamx_visibility_census;
void loamx_default_visibility_params(loamx_visibility_params* p);
/* Parameter refusals of every entry point below. LOAMX_ERR_BAD_PARAM: a non-finite double, min_range < 0, max_range < min_range,
 * margin < 0, margin_rel < 0, through_ratio < 0. LOAMX_ERR_UNSUPPORTED: window_lines > 3 or window_cols > 3. */
/* The votes of n_points device-resident map points (double, world frame, point_stride scalars apart: what loamx_cloud_map_emit_dev
 * writes) over n_scans device-resident organised scans of the layout's shape (n_scans x H W x 3 scalars, double or _f32 float) at
 * d_poses (DEVICE, n_scans x 7: what loamx_compose_trajectory_dev and loamx_pose_graph_optimize_dev leave). accumulate == 0: every
 * entry of d_votes is written; 1: the counts are added to what d_votes holds (a drive in several calls). Asynchronous on the
 * context's stream; synchronises only when the workspace has to grow. LOAMX_ERR_BAD_PARAM: a null layout, params, d_votes, d_points
 * or d_scans, point_stride < 3, a layout of another device, a null d_poses with scans; LOAMX_ERR_UNSUPPORTED: 2^32 points or more,
 * 2^31 scans or more, a point_stride beyond 32 bits. A refused call writes nothing. n_points == 0 or n_scans == 0: LOAMX_OK, and
 * with accumulate == 0 the votes are zeroed (the pointers of what is absent may then be NULL).
 *
 * Kernels (loam_amd/csrc/visibility_kernels.hip): one map point per thread, the scans dealt over workgroup rows of 32 (more when
 * there are more than 65535 x 32 scans); the layout's two tables are staged in LDS when they fit 48 KB; the range test comes
 * first; the counts stay in registers and leave as one store per point (one row, no accumulation) or one integer atomic per
 * non-zero field. A first launch writes every cell's squared range (negative: not usable) into grow-on-demand workspace (8 bytes
 * per cell of the call's scans) and the window reads 8 bytes per cell. Context option NO_VISIBILITY_RANGES: no first launch, the
 * window reads the scans' points and squares them itself — the same bytes, no workspace, 1.27 times the time on the drive of
 * tools/bench_visibility.py. */
int loamx_visibility_votes_dev(loamx_ctx* ctx, const loamx_scan_layout* layout, const double* d_points, size_t point_stride, size_t n_points,
                               const double* d_scans, size_t n_scans, const double* d_poses, const loamx_visibility_params* params,
                               int accumulate, loamx_visibility_tally* d_votes);
int loamx_visibility_votes_dev_f32(loamx_ctx* ctx, const loamx_scan_layout* layout, const double* d_points, size_t point_stride, size_t n_points,
                                   const float* d_scans, size_t n_scans, const double* d_poses, const loamx_visibility_params* params,
                                   int accumulate, loamx_visibility_tally* d_votes);
/* The decision per point and the ordered compaction of the points that stay (never a sort: kept points keep their input order).
 * Outputs, each may be NULL: d_dynamic_out (uint8 per point, n_points entries, 1 = dynamic); d_static_xyz_out (capacity x 3: the
 * kept points' coordinates, read from d_points; ignored when d_points is NULL); d_static_index_out (capacity: their indices).
 * *d_n_static_out is the number of kept points even when it exceeds capacity; every entry below min(n, capacity) of the two
 * compacted outputs is written and nothing beyond it. Asynchronous; synchronises only when the workspace has to grow.
 * LOAMX_ERR_BAD_PARAM: a null params or d_n_static_out, a null d_votes with points, point_stride < 3 with a non-null d_points, a
 * null d_static_xyz_out with a non-null d_points and capacity > 0; LOAMX_ERR_UNSUPPORTED: 2^32 points or more. A refused call
 * writes nothing. */
int loamx_visibility_filter_dev(loamx_ctx* ctx, const loamx_visibility_tally* d_votes, size_t n_points, const loamx_visibility_params* params,
                                const double* d_points, size_t point_stride, uint8_t* d_dynamic_out, double* d_static_xyz_out,
                                uint32_t* d_static_index_out, size_t capacity, uint32_t* d_n_static_out);
/* host memory in and out, synchronous: votes has n_points entries, all written */
int loamx_visibility_votes(loamx_ctx* ctx, const loamx_scan_layout* layout, const double* points, size_t point_stride, size_t n_points,
                           const double* scans, size_t n_scans, const double* poses, const loamx_visibility_params* params,
                           loamx_visibility_tally* votes);
int loamx_visibility_votes_f32(loamx_ctx* ctx, const loamx_scan_layout* layout, const double* points, size_t point_stride, size_t n_points,
                               const float* scans, size_t n_scans, const double* poses, const loamx_visibility_params* params,
                               loamx_visibility_tally* votes);
/* The last votes call of the context (device or host form). Synchronises. LOAMX_ERR_BAD_PARAM before any votes call. Never part of
 * a result. */
int loamx_ctx_last_visibility_census(loamx_ctx* ctx, loamx_visibility_census* out);

/* ---- occupancy map (no reference counterpart; the free / occupied / unknown distinction of OctoMap). The cloud map and the
 * visibility votes say where the sensor hit something; this map also says where it saw nothing. A device-resident hash table
 * voxel -> (hits, passes), two integer counts per voxel, filled by walking every beam from the sensor's position to its return.
 * Counts are integer sums and the walk of a ray depends on that ray alone, so every schedule, every split over workgroups and every
 * split of a drive into calls gives the same bytes; a numpy model is compared by equality (tests/occupancy_common.py). It is read
 * back through three forms whose order is dense or given by the caller (points, a 3-D box, a 2-D slice): nothing is ever sorted.
 *
 * The rule (loam_amd/csrc/occupancy_math.h). FP64 throughout, float input widened first; every product, quotient, sum and
 * difference is one operation rounded on its own, in the order written; the only libm call is sqrt; min2 = min_range^2 and
 * max2 = max_range^2 are formed once by the host. Per ray, for point p of cloud c whose pose (q, t) is read from DEVICE memory
 * (no pose array: p' = p, o = 0):
 *   1 validity   the cloud map's tests on p and r2 = x x + y y + z z. Not finite: counted `invalid`, dropped. !(r2 >= min2): counted
 *                `range_short`, dropped (this removes the (0, 0, 0) cells). !(r2 <= max2): counted `range_long`; with clip_long
 *                the ray is LONG: it is walked up to max_range and makes no hit; without, it is dropped.
 *   2 end points p' = pose.act(p) (the cloud map's function), o = t, d = p' - o per axis, dist = sqrt(r2);
 *                s = (dist - end_margin) / dist for a normal ray, s = max_range / dist for a long one. !(s > 0): the ray has its
 *                hit and no walk. Walk end e = o + s d per axis: one product, one sum.
 *   3 hit        a normal ray's hit voxel is the voxel of p' by the cloud map's rule (floor(p' / leaf), |v| < 2^20, the same
 *                key: at equal leaf an occupancy key is a cloud-map key). p' outside that range: the ray is counted `outside`
 *                and dropped whole. Otherwise hits[key] += 1 and the ray counts in `rays_hit`.
 *   4 walk       per axis a: to = o[a] / leaf, te = e[a] / leaf, v = floor(to), ve = floor(te). Either outside |v| < 2^20 on any
 *                axis: counted `outside`, no walk (the hit stays). rem[a] = |ve - v|, dir[a] = +-1. Where rem[a] > 0:
 *                ad = |te - to|, tDelta[a] = 1.0 / ad, tMax[a] = (dir > 0 ? (v + 1.0) - to : to - v) / ad. The start voxel is
 *                visited, then exactly rem[0] + rem[1] + rem[2] steps follow; in each, among the axes with rem[a] > 0 the one with
 *                the smallest tMax is taken (ties: the lowest axis), v[a] += dir[a], tMax[a] = tMax[a] + tDelta[a], rem[a] -= 1,
 *                and v is visited. The walk ends in ve and its length is known before it starts. Every visited voxel whose key
 *                differs from the ray's own hit key takes passes += 1 and counts in `visits`.
 *                THIS is the definition of the visited set, not "the voxels the segment meets" (they differ by roundings at faces).
 *   5 state      OCCUPIED iff hits >= min_hits && (double) hits >= occ_ratio * (double) passes; otherwise FREE iff
 *                passes >= min_passes; otherwise UNKNOWN, which includes a voxel without a slot. With occ_ratio 0 a hit always
 *                wins; raise it to let passes erase hits. A hit of one scan is not shielded from the passes of the same scan
 *                (OctoMap's per-scan priority would make the result depend on how a drive is split into calls): occ_ratio and
 *                end_margin are the knobs instead.
 * Storage. One device block per map, allocated at create and never grown: 2^k >= 2 max_voxels slots of a 64-bit key (all ones:
 *   empty) and one 64-bit count word hits << 32 | passes, and the counters. A visit is one 64-bit compare-and-swap probe whose
 *   returned value decides plus ONE 64-bit atomic add. At most 2^32 - 2 rays may be offered between two clears, so neither half
 *   of a word can wrap (a ray visits no voxel twice).
 * Overflow. `overflow` counts the visits and hits whose probe gave up after 2^k slots (they were added nowhere). FROM THE FIRST
 *   OVERFLOW UNTIL THE NEXT CLEAR the map promises only that every call returns and that the stats say so.
 * Kernels (loam_amd/csrc/occupancy_kernels.hip). One ray per lane; the lanes of a wavefront are neighbouring beams, and in every
 *   step of the walk runs of neighbouring lanes that stand in the same voxel are combined into one claim that adds the run's
 *   length (the hit goes the same way). Context option NO_OCCUPANCY_COMBINE: one claim per visit; the same bytes.
 *   loamx_occupancy_claims_read tells the two apart. */
enum { LOAMX_OCC_UNKNOWN = 0, LOAMX_OCC_FREE = 1, LOAMX_OCC_OCCUPIED = 2 };
typedef struct {
  double leaf;         /* 0.2 */
  double min_range;    /* 0.5 */
  double max_range;    /* 80.0 */
  double end_margin;   /* 0.2 */
  uint32_t clip_long;  /* 1 */
  uint32_t min_hits;   /* 1 */
  double occ_ratio;    /* 0.0 */
  uint32_t min_passes; /* 1 */
} loamx_occupancy_params;
typedef struct {
  uint64_t rays_offered; /* since the last clear, dropped ones included */
  uint64_t rays_hit;     /* rays that made a hit */
  uint64_t invalid, range_short, range_long, outside;
  uint64_t visits;       /* passes made */
  uint64_t voxels;       /* empty slots won: the voxels of the table */
  uint64_t overflow;
} loamx_occupancy_stats;
/* A map belongs to the context it was created on: every other entry point refuses it on another context (LOAMX_ERR_BAD_PARAM).
 * The context's mutex and stream put its uses in order. */
typedef struct loamx_occupancy_map loamx_occupancy_map;
void loamx_default_occupancy_params(loamx_occupancy_params* p);
/* LOAMX_ERR_BAD_PARAM: a null argument, leaf not finite or <= 0, a negative or non-finite min_range, max_range, end_margin or
 * occ_ratio, max_range < min_range, max_voxels == 0; LOAMX_ERR_UNSUPPORTED: max_range / leaf > 4096 (with a unit quaternion this
 * keeps a walk under 3 x 4098 steps), max_voxels > 2^30. */
int loamx_occupancy_create(loamx_ctx* ctx, const loamx_occupancy_params* params, size_t max_voxels, loamx_occupancy_map** out);
void loamx_occupancy_destroy(loamx_ctx* ctx, loamx_occupancy_map* map);
/* an empty map again. Asynchronous on the context's stream. */
int loamx_occupancy_clear(loamx_ctx* ctx, loamx_occupancy_map* map);
/* The arguments, conventions and refusals of loamx_cloud_map_add_clouds_dev, so that the two are called side by side on the same
 * buffers: n_clouds device-resident clouds back to back, cloud_offsets a HOST array of n_clouds + 1 entries, d_poses DEVICE
 * n_clouds x 7 or NULL. Asynchronous, no host round trip. LOAMX_ERR_UNSUPPORTED: more than 2^32 - 2 rays offered since the last
 * clear with this call's. A refused call changes nothing. */
int loamx_occupancy_add_clouds_dev(loamx_ctx* ctx, loamx_occupancy_map* map, const double* d_points, size_t point_stride,
                                   const size_t* cloud_offsets, size_t n_clouds, const double* d_poses);
int loamx_occupancy_add_clouds_dev_f32(loamx_ctx* ctx, loamx_occupancy_map* map, const float* d_points, size_t point_stride,
                                       const size_t* cloud_offsets, size_t n_clouds, const double* d_poses);
/* The counts and the state of the voxel of each of n device-resident points (double, map frame, point_stride scalars apart), the
 * voxel found by the cloud map's rule: d_counts_out[i] = (hits, passes), d_state_out[i] = LOAMX_OCC_*; either may be NULL. No
 * voxel or no slot: (0, 0) and UNKNOWN. Fed with what loamx_cloud_map_emit_dev wrote, it labels that map's centroids in its own
 * order. The map is not changed. Asynchronous. LOAMX_ERR_BAD_PARAM: a null map, null points with n > 0, point_stride < 3;
 * LOAMX_ERR_UNSUPPORTED: n > 2^31, a point_stride beyond 32 bits. */
int loamx_occupancy_query_dev(loamx_ctx* ctx, const loamx_occupancy_map* map, const double* d_points, size_t point_stride, size_t n,
                              uint32_t* d_counts_out /* [n][2] */, uint8_t* d_state_out /* [n] */);
/* A dense box of voxels vmin .. vmin + dims - 1, x fastest: entry (z dims[1] + y) dims[0] + x. Voxels outside |v| < 2^20 read as
 * without a slot. Either output may be NULL. Asynchronous. LOAMX_ERR_BAD_PARAM: a null map, vmin or dims; LOAMX_ERR_UNSUPPORTED:
 * more than 2^31 voxels. A box with a dimension of 0 writes nothing. */
int loamx_occupancy_box_dev(loamx_ctx* ctx, const loamx_occupancy_map* map, const int32_t vmin[3], const uint32_t dims[3],
                            uint32_t* d_counts_out, uint8_t* d_state_out);
/* The 2-D grid a planner takes, d_grid_out[y dims[0] + x]: column (x, y) of the same box is OCCUPIED if any voxel of its dims[2]
 * levels is, otherwise FREE if any is, otherwise UNKNOWN. Asynchronous. Refusals as the box's, and a null d_grid_out with columns. */
int loamx_occupancy_slice_dev(loamx_ctx* ctx, const loamx_occupancy_map* map, const int32_t vmin[3], const uint32_t dims[3],
                              uint8_t* d_grid_out /* [dims[1]][dims[0]] */);
/* synchronises */
int loamx_occupancy_stats_read(loamx_ctx* ctx, const loamx_occupancy_map* map, loamx_occupancy_stats* out);
/* Measurement read-out: the claims since the last clear, that is, how often the walk kernel began a probe: once per hit and per
 * pass without combining, once per run of a wavefront with it. Changes nothing; synchronises. */
int loamx_occupancy_claims_read(loamx_ctx* ctx, const loamx_occupancy_map* map, uint64_t* claims);
/* host forms, synchronous: one cloud in host memory with a HOST pose (NULL = no transform); the read-outs from and to host arrays */
int loamx_occupancy_add_cloud(loamx_ctx* ctx, loamx_occupancy_map* map, const double* points, size_t point_stride, size_t n_points,
                              const double pose[7]);
int loamx_occupancy_add_cloud_f32(loamx_ctx* ctx, loamx_occupancy_map* map, const float* points, size_t point_stride, size_t n_points,
                                  const double pose[7]);
int loamx_occupancy_query(loamx_ctx* ctx, const loamx_occupancy_map* map, const double* points, size_t point_stride, size_t n,
                          uint32_t* counts_out, uint8_t* state_out);
int loamx_occupancy_box(loamx_ctx* ctx, const loamx_occupancy_map* map, const int32_t vmin[3], const uint32_t dims[3], uint32_t* counts_out,
                        uint8_t* state_out);
int loamx_occupancy_slice(loamx_ctx* ctx, const loamx_occupancy_map* map, const int32_t vmin[3], const uint32_t dims[3], uint8_t* grid_out);

/* ---- occupancy distance field (no reference counterpart; the ESDF of voxblox and nvblox, truncated). What a planner takes from
 * an occupancy map is clearance: per voxel of a box, or per column of a slice, the exact Euclidean distance to the nearest
 * obstacle voxel and the direction to it. The field is integer and exact, so every schedule gives the same bytes and a numpy model
 * is compared by equality (tests/distance_common.py). The rule is executable in loam_amd/csrc/distance_math.h (host + device);
 * tests/hostcheck_distance compares a g++ build of it with the model.
 *   obstacle   a voxel is an obstacle iff its state is OCCUPIED, or, with unknown_is_obstacle, UNKNOWN. The state of a voxel is
 *              the one loamx_occupancy_box_dev writes: step 5 of the occupancy map on the voxel's counts, (0, 0) for a voxel
 *              without a slot and for a voxel outside |v| < 2^20, which reads as without a slot. With the usual thresholds
 *              (min_hits >= 1, min_passes >= 1) both are UNKNOWN. The slice: column (x, y) takes the state
 *              loamx_occupancy_slice_dev gives it over its dims[2] levels, and the field is 2-D over columns.
 *   field      R = max_dist_voxels, 1 <= R <= 255. For a voxel v of the box, D(v) is the minimum of |w - v|^2, the integer sum of
 *              the squared offsets, over ALL obstacle voxels w of the lattice, those outside the box included: the map is read
 *              in a halo of R voxels around the box on every axis (the slice: on x and y), so a window that follows the robot has
 *              no edge artefacts. d2(v) = D(v) if D(v) <= R^2, otherwise LOAMX_DIST_FAR = 0xFFFF; R^2 <= 65025 < 0xFFFF. An
 *              obstacle voxel has d2 = 0.
 *   nearest    offset(v) = w* - v per axis, where w* is the minimiser with the LOWEST LINEAR INDEX, x fastest: the lowest z, then
 *              the lowest y, then the lowest x. (0, 0, 0) where d2 is 0 or LOAMX_DIST_FAR. The slice has two components (x, y).
 *   metres     (float)(sqrt((double) d2) * leaf), each operation rounded on its own; +inf for LOAMX_DIST_FAR.
 * Truncation stays exact: if D(v) <= R^2 the minimiser lies within +-R on every axis, so three separable passes x, y, z over
 * windows of +-R find it, and every intermediate above R^2 may be dropped as "none". Ties of the passes go to the lower
 * coordinate (x-pass: the lower x; y-pass: the lower y'; z-pass: the lower z'), which yields exactly the minimiser named above.
 * Layout: that of loamx_occupancy_box_dev (entry (z dims[1] + y) dims[0] + x) and of loamx_occupancy_slice_dev (y dims[0] + x);
 * offsets are 3 (slice: 2) int16 per entry. Each of the three outputs may be NULL. A box with a dimension of 0 writes nothing (the
 * slice: dims[0] or dims[1]; with dims[2] == 0 every column is UNKNOWN).
 * Kernels (loam_amd/csrc/distance_kernels.hip): a bit mask of the extended box, one wavefront's ballot per 64-bit word (the only
 * launch that reads the table); the x-pass on the mask words by count-leading / count-trailing zeros; the y-pass and the z-pass one
 * voxel per lane, walking outwards and stopping as soon as k^2 exceeds the best found, so the cost follows the distance found and
 * not R. Context option NO_DISTANCE_EARLY_EXIT: the whole window is walked; the same bytes. No atomics, nothing read back.
 * The device forms enqueue on the context's stream and return. The mask and the pass intermediates belong to the handle: they are
 * allocated at the handle's first distance call, grown when a call needs more (such a call may wait on the allocator and the
 * stream) and freed at destroy; every call that fits only enqueues. The map's table is only read. A refused call changes nothing,
 * outputs included.
 * LOAMX_ERR_BAD_PARAM: a null map, vmin, dims or params, max_dist_voxels == 0, a map of another context. LOAMX_ERR_UNSUPPORTED:
 * max_dist_voxels > 255; more than 2^31 voxels in the EXTENDED box (dims + 2R per axis; the slice: dims[0] + 2R by dims[1] + 2R
 * columns). LOAMX_ERR_HIP: the allocation of the staging failed. */
#define LOAMX_DIST_FAR 0xFFFFu
typedef struct {
  uint32_t max_dist_voxels;     /* 10 */
  uint32_t unknown_is_obstacle; /* 0 */
} loamx_distance_params;
void loamx_default_distance_params(loamx_distance_params* p);
int loamx_occupancy_distance_box(loamx_ctx* ctx, loamx_occupancy_map* map, const int32_t vmin[3], const uint32_t dims[3],
                                 const loamx_distance_params* params, uint16_t* d_d2_out /* [n] */, int16_t* d_offset_out /* [n][3] */,
                                 float* d_metres_out /* [n] */);
int loamx_occupancy_distance_slice(loamx_ctx* ctx, loamx_occupancy_map* map, const int32_t vmin[3], const uint32_t dims[3],
                                   const loamx_distance_params* params, uint16_t* d_d2_out /* [dims[1]][dims[0]] */,
                                   int16_t* d_offset_out /* [.][2] */, float* d_metres_out);
/* host forms, synchronous: the same fields to host arrays */
int loamx_occupancy_distance_box_host(loamx_ctx* ctx, loamx_occupancy_map* map, const int32_t vmin[3], const uint32_t dims[3],
                                      const loamx_distance_params* params, uint16_t* d2_out, int16_t* offset_out, float* metres_out);
int loamx_occupancy_distance_slice_host(loamx_ctx* ctx, loamx_occupancy_map* map, const int32_t vmin[3], const uint32_t dims[3],
                                        const loamx_distance_params* params, uint16_t* d2_out, int16_t* offset_out, float* metres_out);

/* ---- occupancy ray casting (no reference counterpart; OctoMap's castRay). "What does a ray from here meet first?": line of sight
 * and segment collision for a planner, and the scan the map predicts at a pose, to lay beside the scan that arrived. A ray is a
 * segment from o to e in the map frame, three doubles each. The result is integer or individually rounded FP64 and depends on that
 * ray alone, so every schedule gives the same bytes and a Python model is compared by equality (tests/raycast_common.py). The rule
 * is executable in loam_amd/csrc/raycast_math.h (host + device); tests/hostcheck_raycast compares a g++ build of it with the model.
 * FP64 throughout; every product, quotient, sum and difference is one operation rounded on its own; no libm call.
 *   1 validity   a coordinate of o or e that is not finite: status INVALID, no walk.
 *   2 walk       step 4 of the occupancy map on (o, e), unchanged: the same set-up, the same pick, the same ties. A voxel coordinate
 *                of o or e outside |v| < 2^20: status OUTSIDE, no walk. Otherwise the start voxel is visit 0 and up to
 *                rem[0] + rem[1] + rem[2] steps follow.
 *   3 parameters t_enter of visit 0 is 0.0; of every other visit it is the tMax that was picked in the step that led into the
 *                voxel, before that step advanced it. t_exit of a visit is the smallest tMax among the axes with rem > 0 on arrival,
 *                1.0 if no axis has steps left. So t_exit of visit k and t_enter of visit k + 1 are the same double.
 *   4 test       visits with index < skip_start are walked but not tested (a ray that starts on a surface). For every other visit
 *                the voxel's count word is read (a voxel without a slot: (0, 0)) and step 5 of the occupancy map gives its state
 *                under the map's own thresholds. OCCUPIED: stop, status HIT. UNKNOWN with unknown_stops != 0: stop, status UNKNOWN.
 *                UNKNOWN with unknown_stops == 0: n_unknown += 1 and on. FREE: on.
 *   5 cap        the walk takes at most max_steps steps (default 3 x 4098, the bound of a walk of the map's own add; above 2^22:
 *                LOAMX_ERR_UNSUPPORTED). A visit that did not stop with no step left in the walk: status CLEAR (the ray ended in
 *                e's voxel). Otherwise, with the cap used up: status TRUNCATED. Segment lengths are device data that the host
 *                cannot refuse; the cap is what bounds a lane's time.
 *   6 record     40 bytes, every byte written for every ray: status, visits (voxels visited, the last one included), the voxel the
 *                ray stopped or ended in, n_unknown, t_enter and t_exit of that voxel. OUTSIDE and INVALID: zeros behind the status.
 * Rendered scans. d_dirs: n_beams x 3 doubles, the unit directions of the beams in the sensor frame in the scan's cell order; the
 *   caller supplies them (the scan layout stores cell boundaries, not centres), so no cos or sin runs in the library. d_poses:
 *   n_poses x 7 in DEVICE memory (qx qy qz qw tx ty tz). Beam b of pose i is the segment from o = t_i to
 *   e = pose_i.act((max_range d.x, max_range d.y, max_range d.z)), cast by the rule above; a pose with an entry that is not finite
 *   makes all of its beams INVALID. On HIT tau = t_enter (LOAMX_RAY_AT_ENTER) or 0.5 * (t_enter + t_exit) (LOAMX_RAY_AT_MIDDLE),
 *   range = tau * max_range and the point is (range d.x, range d.y, range d.z) in the sensor frame. Every other status: range 0 and
 *   the point (+0, +0, +0), the "no return" cell of the organiser, so d_scans_out (n_poses x n_beams x 3 doubles) goes straight
 *   into the extraction, the place descriptors and the visibility votes. The range is a voxel's entry or middle: it is quantised
 *   to the leaf. hit_at is used by this form only.
 * Kernels (loam_amd/csrc/raycast_kernels.hip). One ray per lane, 256 threads; the lanes of a wavefront are neighbouring rays or
 *   beams in input order, and the wavefront loops while any lane has a voxel to visit. In every trip every lane that tests its
 *   voxel looks it up. Context option RAYCAST_COMBINE: runs of neighbouring lanes that test the same voxel make ONE look-up, the
 *   head of the run probes the table and the others take the count word from it; the same bytes, only `probes` differs. Measured,
 *   the two forms are level and the plain one a little faster, so it is the default. The table is only
 *   read. Both device forms enqueue on the context's stream and return; nothing is read back. A refused call writes nothing.
 * Census. loamx_ctx_last_raycast_census reads back (it synchronises) the counters of the context's last cast or render call:
 *   rays, visits (the TESTED visits: those that needed a count word), probes (look-ups made: equal to visits without combining),
 *   and the rays by status. A call with no ray leaves all zero.
 * LOAMX_ERR_BAD_PARAM: a null map or params, a map of another context, null origins, ends or records with n > 0, stride < 3,
 *   an unknown hit_at; the render: null d_dirs or d_poses with rays, max_range not finite or <= 0. LOAMX_ERR_UNSUPPORTED:
 *   max_steps > 2^22, n > 2^31 (the render: n_poses x n_beams > 2^31), a stride beyond 32 bits. No ray: LOAMX_OK, nothing written. */
enum { LOAMX_RAY_CLEAR = 0, LOAMX_RAY_HIT = 1, LOAMX_RAY_UNKNOWN = 2, LOAMX_RAY_TRUNCATED = 3, LOAMX_RAY_OUTSIDE = 4, LOAMX_RAY_INVALID = 5 };
enum { LOAMX_RAY_AT_ENTER = 0, LOAMX_RAY_AT_MIDDLE = 1 };
typedef struct {
  uint32_t skip_start;    /* 0 */
  uint32_t unknown_stops; /* 0 */
  uint32_t max_steps;     /* 3 x 4098 */
  uint32_t hit_at;        /* LOAMX_RAY_AT_MIDDLE */
} loamx_raycast_params;
typedef struct {
  uint32_t status; /* LOAMX_RAY_* */
  uint32_t visits;
  int32_t voxel[3];
  uint32_t n_unknown;
  double t_enter, t_exit;
} loamx_ray_record;
typedef struct {
  uint64_t rays, visits, probes;
  uint64_t hit, unknown, clear, truncated, outside, invalid;
} loamx_raycast_census;
void loamx_default_raycast_params(loamx_raycast_params* p);
/* n segments in DEVICE memory, segment i from d_origins + i stride to d_ends + i stride (doubles); one record each */
int loamx_occupancy_cast_rays(loamx_ctx* ctx, const loamx_occupancy_map* map, const double* d_origins, const double* d_ends, size_t stride, size_t n,
                              const loamx_raycast_params* params, loamx_ray_record* d_records_out /* [n] */);
/* the expected scans of the map: ray (i, b) at index i n_beams + b of every output; each output may be NULL */
int loamx_occupancy_render_scans(loamx_ctx* ctx, const loamx_occupancy_map* map, const double* d_dirs /* [n_beams][3] */, size_t n_beams,
                                 const double* d_poses /* [n_poses][7] */, size_t n_poses, double max_range, const loamx_raycast_params* params,
                                 double* d_scans_out /* [n_poses][n_beams][3] */, double* d_ranges_out /* [n_poses][n_beams] */,
                                 loamx_ray_record* d_records_out /* [n_poses][n_beams] */);
/* host forms, synchronous: host arrays in and out */
int loamx_occupancy_cast_rays_host(loamx_ctx* ctx, const loamx_occupancy_map* map, const double* origins, const double* ends, size_t stride, size_t n,
                                   const loamx_raycast_params* params, loamx_ray_record* records_out);
int loamx_occupancy_render_scans_host(loamx_ctx* ctx, const loamx_occupancy_map* map, const double* dirs, size_t n_beams, const double* poses,
                                      size_t n_poses, double max_range, const loamx_raycast_params* params, double* scans_out, double* ranges_out,
                                      loamx_ray_record* records_out);
/* synchronises */
int loamx_ctx_last_raycast_census(loamx_ctx* ctx, loamx_raycast_census* out);

/* ---- surfel map (no reference counterpart; the per-voxel Gaussians of NDT, the surfels of a point-to-plane map). What the
 * consumers of a map need beyond a centroid: per voxel the mean, the covariance, its eigenvalues and the normal, turned towards
 * where the voxel was seen from. The inputs are the cloud map's; the sums are integers, so every schedule and every partial
 * combine gives the same bytes, and a Python model is compared by equality (tests/surfel_common.py). The rule is executable in
 * loam_amd/csrc/surfel_math.h; every product, quotient, sum and difference is rounded on its own, in the order written, and sqrt is
 * the only libm call.
 *
 * Per point p of cloud c:
 *   1 validity   the cloud map's (`invalid`, `range`).
 *   2 transform  p' = pose_c.act(p), pose_c from DEVICE memory; no pose array: p' = p.
 *   3 voxel      the cloud map's key and 32-bit offsets u at the map's leaf (|v| < 2^20, otherwise `outside`): at equal leaf a surfel
 *                key IS a cloud-map key.
 *   4 offsets    q[a] = u[a] >> 16: 16 bits, steps of leaf / 65536. A product q[a] q[b] < 2^32 and at most 2^32 - 2 points are
 *                offered between two clears, so no 64-bit sum below can wrap (the width is derived, not tuned).
 *                s[a] += q[a] (3 words, each < 2^48); S[ab] += q[a] q[b], ab = xx xy xz yy yz zz (6 words); count += 1;
 *                first = min(first, g), g the running index exactly as the cloud map defines it.
 *   5 view       o = the translation of pose_c (0 without poses); x[a] = ((o[a] - p'[a]) / leaf) 256.0, then x = -2^30 unless
 *                x >= -2^30, x = 2^30 if x > 2^30 (FP64), w[a] = (int64) floor(x); W[a] += w[a]: three signed 64-bit words,
 *                |W| < 2^62. The clamp keeps a non-unit quaternion or a far-away pose from wrapping a sum.
 * The record of a voxel, surfel_finish(key, s, S, W, count, first, leaf), with dn = (double) count, h = leaf / 65536.0:
 *   mean[a]  = ((double) v[a] + ((double) s[a] / dn) / 65536.0) leaf.
 *   N[ab]    = count S[ab] - s[a] s[b], EXACT in 128-bit integers (each term < 2^96), to FP64 as
 *              sign ((double) hi 18446744073709551616.0 + (double) lo) of the magnitude's two 64-bit halves.
 *   cov[ab]  = (N[ab] / (dn dn)) (h h): the population covariance (S / n - mean^2 in FP64 would cancel for a thin wall far
 *              from the voxel's corner, which is why the numerator is formed in integers).
 *   eigen    the cyclic Jacobi of the registration's line fit: rotations (0,1), (0,2), (1,2) per sweep, at most 32 sweeps, stops when
 *              the three off-diagonals are exactly 0. Eigenvalues ascending by a stable sort of three (ties keep column order),
 *              not clamped at 0. normal = the column of the smallest.
 *   facing   dot = n0 (double) W0 + n1 (double) W1 + n2 (double) W2, left to right. The normal is negated when dot < 0; when
 *              dot == 0 it is negated if its component of largest magnitude is negative (the lowest axis on ties). A voxel of
 *              one point has cov = 0 and gets what this gives (the x axis, turned): defined, not special-cased.
 * Voxel order, storage, overflow and ownership are the cloud map's: the voxels are listed in order of first appearance (a list of
 * slots appended to, never sorted); a table of 2^k >= 2 max_voxels slots (key, first, twelve 64-bit sums and count: 112 B each),
 * the list and the scratch of one round of launches are allocated at create and never grown; `overflow` counts as there, and
 * FROM THE FIRST OVERFLOW UNTIL THE NEXT CLEAR only "every call returns and the stats say so" is promised. A map belongs to the
 * context it was created on. Context option NO_SURFEL_COMBINE: one claim per used point instead of one per run of a wavefront;
 * the same bytes.
 *
 * NAMES. On this handle the plain name is the device form (asynchronous on the context's stream, no host wait) and the host
 * forms carry _host. */
typedef struct {
  double mean[3];
  double cov[6];    /* xx xy xz yy yz zz */
  double eval[3];   /* ascending */
  double normal[3]; /* unit, towards the sensor positions */
  uint32_t count, first;
} loamx_surfel; /* 128 bytes */
typedef struct {
  double leaf;      /* 0.5 */
  double min_range; /* 0.5 */
  double max_range; /* 120.0 */
} loamx_surfel_map_params;
typedef struct {
  uint64_t voxels, points_offered, points_used, invalid, range, outside, overflow;
} loamx_surfel_map_stats;
typedef struct loamx_surfel_map loamx_surfel_map;
void loamx_default_surfel_map_params(loamx_surfel_map_params* p);
/* the refusals of loamx_cloud_map_create */
int loamx_surfel_map_create(loamx_ctx* ctx, const loamx_surfel_map_params* params, size_t max_voxels, loamx_surfel_map** out);
void loamx_surfel_map_destroy(loamx_ctx* ctx, loamx_surfel_map* map);
/* an empty map again, running index 0. Asynchronous. */
int loamx_surfel_map_clear(loamx_ctx* ctx, loamx_surfel_map* map);
/* the arguments, conventions and refusals of loamx_cloud_map_add_clouds_dev (DEVICE points and poses, HOST cloud_offsets).
 * Asynchronous; a refused call changes nothing. */
int loamx_surfel_map_add_clouds(loamx_ctx* ctx, loamx_surfel_map* map, const double* d_points, size_t point_stride,
                                const size_t* cloud_offsets, size_t n_clouds, const double* d_poses);
int loamx_surfel_map_add_clouds_f32(loamx_ctx* ctx, loamx_surfel_map* map, const float* d_points, size_t point_stride,
                                    const size_t* cloud_offsets, size_t n_clouds, const double* d_poses);
/* The voxels with count >= min_points in list order, to DEVICE memory: the records (d_out, capacity), the means (d_xyz_out,
 * capacity x 3) and the normals (d_normal_out, capacity x 3); each of the three may be NULL. *d_n_out is the number that qualify
 * even beyond capacity; every entry below min(n, capacity) of each non-null output is written and nothing beyond. Asynchronous.
 * LOAMX_ERR_BAD_PARAM: a null map or d_n_out. */
int loamx_surfel_map_emit(loamx_ctx* ctx, const loamx_surfel_map* map, uint32_t min_points, loamx_surfel* d_out, double* d_xyz_out,
                          double* d_normal_out, size_t capacity, uint32_t* d_n_out);
/* Per device-resident point (double, map frame, point_stride scalars apart): the record of its voxel, the signed distance
 * normal . (p - mean) evaluated left to right, and the voxel's count; each output may be NULL. A point without a voxel (not
 * finite, |v| >= 2^20, no slot) or in a voxel with count < min_points: a record of zero bytes, distance 0.0, count 0. Asynchronous.
 * LOAMX_ERR_BAD_PARAM: a null map, null points with n_points > 0, point_stride < 3; LOAMX_ERR_UNSUPPORTED: n_points > 2^31, a
 * point_stride beyond 32 bits. */
int loamx_surfel_map_query(loamx_ctx* ctx, const loamx_surfel_map* map, const double* d_points, size_t point_stride, size_t n_points,
                           uint32_t min_points, loamx_surfel* d_out, double* d_distance_out, uint32_t* d_count_out);
/* synchronise */
int loamx_surfel_map_stats_read(loamx_ctx* ctx, const loamx_surfel_map* map, loamx_surfel_map_stats* out);
/* the claims since the last clear: probes begun by the accumulate kernel, each followed by its fourteen atomics */
int loamx_surfel_map_claims_read(loamx_ctx* ctx, const loamx_surfel_map* map, uint64_t* claims);
/* host forms, synchronous: one cloud in host memory with a HOST pose (NULL = no transform); the records to a host array */
int loamx_surfel_map_add_cloud_host(loamx_ctx* ctx, loamx_surfel_map* map, const double* points, size_t point_stride, size_t n_points,
                                    const double pose[7]);
int loamx_surfel_map_add_cloud_host_f32(loamx_ctx* ctx, loamx_surfel_map* map, const float* points, size_t point_stride, size_t n_points,
                                        const double pose[7]);
int loamx_surfel_map_emit_host(loamx_ctx* ctx, const loamx_surfel_map* map, uint32_t min_points, loamx_surfel* out, size_t capacity,
                               size_t* n_out);

/* ---- surfel localisation (no reference counterpart; the point-to-plane scan-to-map step of SuMa, VoxelMap and the NDT family).
 * Places clouds in a surfel map: association is a hash lookup of the voxel's fitted plane, so it takes any cloud (a full scan, an
 * unordered cloud, the planar features alone) and needs no k-NN index. The whole solve stays on the device: a call enqueues
 * 1 + 2 max_iterations + 2 launches per group of 256 clouds and reads nothing back, so add -> localise the next scan -> add it at
 * the localised pose runs without a synchronise. The rule is executable in loam_amd/csrc/localize_math.h (host + device,
 * every operation rounded on its own in the order written, sqrt the only libm call); a g++ build of it (tests/hostcheck_localize)
 * runs the solve in the kernels' orders and is compared with the device by bytes.
 *
 * One evaluation of cloud c at the pose T = map_T_cloud (7 doubles, x y z w tx ty tz), per point p:
 *   1 validity    the cloud map's, with the MAP's ranges; a point that fails is counted in n_unused.
 *   2 move        v = T.act(p).
 *   3 home voxel  the cloud map's cell of v at the map's leaf; a point without one (not finite, |v| >= 2^20) is counted in n_unused.
 *   4 candidates  the home voxel; with neighborhood == 7 the six face neighbours follow in the order -x, +x, -y, +y, -z, +z. A
 *                 neighbour whose coordinate leaves |v| < 2^20 is skipped. A candidate is USABLE iff it has a slot,
 *                 count >= min_points, eval[1] > 0 and eval[0] <= planarity eval[1] (no division), eval the eigenvalues of
 *                 surfel_finish.
 *   5 choice      the usable candidate with the smallest |v - mean|^2 = dx dx + dy dy + dz dz, summed left to right; on a tie the
 *                 earlier in the order above wins. No usable candidate: counted in n_no_surfel.
 *   6 gate        s = normal . (v - mean), exactly the distance of the surfel map's query; |s| > max_distance: counted in n_gated
 *                 (max_distance == 0 stands for the map's leaf).
 *   7 row         r = |s|, g = copysign(1, s) normal, J = [v x g, g]: the plane row of loamx_reg_information in the same LEFT
 *                 basis, with the subtraction done first (the s of the gate). A row with a non-finite entry is dropped and counted
 *                 in n_unused. Huber at huber_delta: for r > huber_delta, J and r are scaled by sqrt(huber_delta / r) and the row
 *                 is counted in n_huber; huber_delta == 0 switches it off.
 *   8 sums        the upper triangle of J^T J (21), J^T r (6) and r^2 (1) of the scaled rows.
 * Order of the sums, a function of the cloud alone: chunk k of a cloud is its points [4096 k, 4096 (k + 1)); thread t of 256 takes
 * the points t, t + 256, ... of the chunk in that order; a wavefront's 64 values meet in a shuffle-down tree over 32 .. 1; the four
 * wavefronts are added in order; the chunks are added in order. A cloud has the same bytes alone and inside any batch.
 * The solve, per cloud: H = the mirrored triangle, eigenpairs as loamx_reg_information has them. Direction i is USED iff
 * eigenvalue[i] > min_eigenvalue_per_row n_rows (bit i of used_mask); the step is d = - sum over the used i, ascending, of
 * evec_i (evec_i . gradient) / eigenvalue_i (LOAM's degeneracy remapping: a floor-only map moves z, roll and pitch only); the
 * retraction is on the left, T <- (normalise([omega / 2, 1]), t) o T with d = [omega, t]. Plain Gauss-Newton: every evaluation
 * associates anew, there is no trust region. Per iteration, in this order:
 *   0 a non-finite pose           -> LOAMX_LOCALIZE_NOT_FINITE, the pose stays (such a pose gives no row: it is looked at before 1)
 *   1 n_rows < min_rows           -> LOAMX_LOCALIZE_TOO_FEW_ROWS, the pose stays
 *   2 a non-finite d or new pose  -> LOAMX_LOCALIZE_NOT_FINITE, the pose stays
 *   3 the step is applied, iterations += 1; last_rotation = |omega|, last_translation = |t|
 *   4 |omega| < rotation_convergence_thresh && |t| < position_convergence_thresh -> LOAMX_LOCALIZE_CONVERGED
 *   5 iterations == max_iterations -> LOAMX_LOCALIZE_MAX_ITERATIONS
 * Then ONE more evaluation of every cloud at its returned pose fills final_cost, the counters, used_mask and the optional
 * loamx_reg_information record (n_edge = 0, n_plane = n_rows, n_dropped = 0, the eigenpairs of that pass). initial_cost and
 * n_rows_initial are those of the first evaluation. max_iterations == 0 returns the pose bit for bit (termination
 * LOAMX_LOCALIZE_MAX_ITERATIONS) and the information at it. The costs are sums of scaled r^2, not halved.
 * The localiser owns a plane cache of one 64-byte record per table slot (mean, normal, count, usable), rebuilt at the start of every
 * call, so a map that was cleared or added to between two calls is fine. Context option NO_LOCALIZE_PLANES: no cache, every candidate
 * is finished where it is looked at; the same bytes. PRECONDITION: a map that has not overflowed since its last clear. The cache is
 * written for the LISTED voxels; past the first overflow the map holds claimed slots outside its list, whose cache records are
 * whatever an earlier call left, so the two forms may then differ and, as for the map itself, only "every call returns" is promised.
 * WHAT CONVERGED MEANS: the last step was small, not that the pose is right. This is plain Gauss-Newton without a trust region: where
 * the map leaves a direction nearly open (a street seen along its axis, open ground) its eigenvalue can lie just above
 * min_eigenvalue_per_row n_rows, the step along it is large and poorly founded, and a cloud can end metres off and still report
 * LOAMX_LOCALIZE_CONVERGED. A caller gates on used_mask and on the eigenvalues of the information record, not on termination alone. The map is only read. Destroying the map before its localiser is the caller's
 * error. On this handle the plain name is the device form and the host form carries _host. */
enum {
  LOAMX_LOCALIZE_CONVERGED = 0,
  LOAMX_LOCALIZE_MAX_ITERATIONS = 1,
  LOAMX_LOCALIZE_TOO_FEW_ROWS = 2,
  LOAMX_LOCALIZE_NOT_FINITE = 3
};
typedef struct {
  uint32_t neighborhood;              /* 7 (or 1: the home voxel only) */
  uint32_t min_points;                /* 5 */
  double planarity;                   /* 0.1 */
  double max_distance;                /* 0: the map's leaf */
  double huber_delta;                 /* 0.1; 0: no Huber */
  uint32_t max_iterations;            /* 10, at most 1000 */
  uint32_t min_rows;                  /* 100 */
  double rotation_convergence_thresh; /* 1e-3 */
  double position_convergence_thresh; /* 1e-2 */
  double min_eigenvalue_per_row;      /* 1e-3 */
} loamx_localize_params;              /* 64 bytes */
typedef struct {
  double pose[7];
  double initial_cost, final_cost;
  double last_rotation, last_translation; /* of the last applied step; 0 without one */
  uint32_t iterations, termination;
  uint32_t n_rows, n_huber, n_no_surfel, n_gated, n_unused; /* of the evaluation at the returned pose */
  uint32_t used_mask;
  uint32_t n_rows_initial;
  uint32_t reserved;
} loamx_localize_result; /* 128 bytes */
typedef struct loamx_surfel_localizer loamx_surfel_localizer;
void loamx_default_localize_params(loamx_localize_params* p);
/* Everything a call needs is allocated here: the plane cache (64 B per table slot), the partial sums of max_points points and the
 * state of max_clouds clouds. LOAMX_ERR_BAD_PARAM: a null argument, a map of another context, max_clouds == 0;
 * LOAMX_ERR_UNSUPPORTED: max_clouds > 2^24, max_points > 2^32 - 2. */
int loamx_surfel_localizer_create(loamx_ctx* ctx, const loamx_surfel_map* map, size_t max_clouds, size_t max_points,
                                  loamx_surfel_localizer** out);
void loamx_surfel_localizer_destroy(loamx_ctx* ctx, loamx_surfel_localizer* loc);
/* n_clouds device-resident clouds back to back (cloud c = the points cloud_offsets[c] .. cloud_offsets[c + 1] - 1 of d_points,
 * point_stride scalars apart; cloud_offsets in HOST memory), each from its pose d_poses_in[c] in DEVICE memory (the layout
 * loamx_compose_trajectory_dev and loamx_pose_graph_optimize_dev leave). Writes d_poses_out (n_clouds x 7, may equal d_poses_in),
 * d_results (n_clouds records) and, unless NULL, d_info (n_clouds records). Asynchronous on the context's stream, no host wait.
 * A refused call changes nothing. LOAMX_ERR_BAD_PARAM: a null localiser, params, cloud_offsets, d_poses_in, d_poses_out or
 * d_results, null points with points, a localiser of another context, point_stride < 3, neighborhood other than 1 or 7, a
 * non-finite or negative parameter, decreasing offsets. LOAMX_ERR_UNSUPPORTED: n_clouds > max_clouds, more points than
 * max_points, max_iterations > 1000, a point_stride beyond 32 bits. n_clouds == 0: LOAMX_OK. */
int loamx_surfel_localizer_run(loamx_ctx* ctx, loamx_surfel_localizer* loc, const double* d_points, size_t point_stride,
                               const size_t* cloud_offsets, size_t n_clouds, const double* d_poses_in, double* d_poses_out,
                               loamx_localize_result* d_results, loamx_reg_information* d_info, const loamx_localize_params* params);
int loamx_surfel_localizer_run_f32(loamx_ctx* ctx, loamx_surfel_localizer* loc, const float* d_points, size_t point_stride,
                                   const size_t* cloud_offsets, size_t n_clouds, const double* d_poses_in, double* d_poses_out,
                                   loamx_localize_result* d_results, loamx_reg_information* d_info, const loamx_localize_params* params);
/* host form, synchronous: one cloud and one pose in host memory; the pose comes back in result->pose; info may be NULL */
int loamx_surfel_localizer_run_host(loamx_ctx* ctx, loamx_surfel_localizer* loc, const double* points, size_t point_stride, size_t n_points,
                                    const double pose[7], const loamx_localize_params* params, loamx_localize_result* result,
                                    loamx_reg_information* info);
int loamx_surfel_localizer_run_host_f32(loamx_ctx* ctx, loamx_surfel_localizer* loc, const float* points, size_t point_stride, size_t n_points,
                                        const double pose[7], const loamx_localize_params* params, loamx_localize_result* result,
                                        loamx_reg_information* info);

/* ---- map window (no reference counterpart). A mapper runs for as long as the vehicle drives, and max_voxels is fixed at create:
 * a crop removes the voxels of a cloud map, a surfel map or an occupancy map outside a box around a pose, so that a map of fixed
 * size follows the sensor. One rule and one set of kernels (loam_amd/csrc/crop_kernels.hip) serve the three maps. The rule is
 * executable in loam_amd/csrc/crop_math.h (host + device, every operation rounded on its own); tests/hostcheck_crop compares a g++
 * build of it with numpy.
 *
 * d_pose: DEVICE memory, one pose of 7 doubles in the layout loamx_compose_trajectory_dev and the localiser's d_poses_out leave
 * (quaternion first, translation in [4..6]). Only the translation is read: the window stays axis-aligned in the map frame, and a
 * quaternion that is no unit quaternion or a NaN is not looked at. NULL: the centre is (0, 0, 0). With a device pose a crop can
 * follow a pose the host has never seen. lo, hi: HOST values in metres relative to the centre; infinite bounds are allowed.
 * d_counts_out: DEVICE memory or NULL, four words {kept, removed, skipped, 0}.
 *   1 centre   c[a] = d_pose[4 + a], or +0.0 without a pose.
 *   2 skip     if a c[a] is not finite the crop is SKIPPED: the map keeps every byte and the counts are {voxels, 0, 1, 0}. A NaN
 *              pose from a lost localisation does not erase the map.
 *   3 bounds   flo[a] = floor((c[a] + lo[a]) / leaf), fhi[a] = floor((c[a] + hi[a]) / leaf): the cloud map's cell function on the
 *              corners of the box. +-inf stays +-inf.
 *   4 keep     a voxel with the integer cell v (unpacked from its key) is kept iff (double)v[a] >= flo[a] && (double)v[a] <= fhi[a]
 *              on all three axes. Every point of the closed box lies in a kept cell: the box is widened to voxel boundaries, never
 *              narrowed.
 * Because 0.0 + x == x, a caller that folds a host-side centre into lo and hi and passes NULL gets the same bytes; the conveniences
 * of capi.py (crop), of include/loam and of the module loam do exactly that.
 * The cloud map and the surfel map afterwards: the kept voxels keep every byte (key, first, sums or moments, W, count) and their
 * relative order in the list; stats.voxels is `kept`; the running index, points_offered, points_used, the drop counters, overflow
 * and claims are not touched. The room in the list is regained: later adds append behind the kept voxels. A removed voxel that is
 * seen again is a new voxel: it gets the new running index as `first` and goes to the end of the list. Emit, query and the
 * localiser see exactly the map with the removed entries deleted, by bytes. The occupancy map afterwards: the kept voxels keep
 * their hits and passes, stats.voxels is `kept`, every other counter is untouched; query, box and slice read UNKNOWN and (0, 0)
 * where a voxel was removed.
 * A map that has overflowed since its last clear keeps the promise it had: the crop returns, nothing else is specified, and the
 * overflow counter is not reset. The limit of 2^32 - 2 points or rays between two clears stays: a crop does not renumber `first`.
 * Asynchronous on the context's stream, six launches, no host wait, nothing read back. The staging of a crop belongs to the handle:
 * it is allocated at the handle's FIRST crop (that call may wait on the allocator), sized once by max_voxels (the occupancy map: by
 * its table's slots), and freed at destroy; every later crop only enqueues. A refused call changes nothing.
 * LOAMX_ERR_BAD_PARAM: a null map, a map of another context, null lo or hi, lo[a] > hi[a], a NaN bound. LOAMX_ERR_HIP: the
 * allocation of the staging failed. */
int loamx_cloud_map_crop(loamx_ctx* ctx, loamx_cloud_map* map, const double* d_pose, const double lo[3], const double hi[3],
                         uint32_t* d_counts_out);
int loamx_surfel_map_crop(loamx_ctx* ctx, loamx_surfel_map* map, const double* d_pose, const double lo[3], const double hi[3],
                          uint32_t* d_counts_out);
int loamx_occupancy_crop(loamx_ctx* ctx, loamx_occupancy_map* map, const double* d_pose, const double lo[3], const double hi[3],
                         uint32_t* d_counts_out);

/* ---- multi-GPU batch mode (BASELINE configs[3]) ------------------------------------------------
 * The reference has no counterpart (registration-inl.h:11-78 takes everything by value / const-ref: scan pairs are
 * independent units). One process per GPU owns a contiguous block of pair ids and runs the single-GPU entry points
 * on it; the only communication is the gather of the 64-byte loamx_reg_result records, done here with RCCL
 * (ncclAllGather, or grouped ncclBroadcast when the shards are uneven) on the context's stream, asynchronously —
 * it is ordered after the registration kernels that produce the records by the stream itself. */
#define LOAMX_COMM_ID_BYTES 128 /* = NCCL_UNIQUE_ID_BYTES */
typedef struct loamx_comm loamx_comm;
/* contiguous block [first, first + count) of rank `rank`; block sizes differ by at most one */
void loamx_shard_range(size_t total_pairs, int world_size, int rank, size_t* first, size_t* count);
/* rank 0 calls this once and hands the 128 bytes to every rank out of band (file, socket, launcher) */
int loamx_comm_get_unique_id(unsigned char id_out[LOAMX_COMM_ID_BYTES]);
/* collective over all ranks: ncclCommInitRank on the context's device */
int loamx_comm_create(loamx_ctx* ctx, const unsigned char id[LOAMX_COMM_ID_BYTES], int world_size, int rank,
                      loamx_comm** out);
/* adopts a communicator the host already owns (an ncclComm_t); loamx_comm_destroy then leaves it alone */
int loamx_comm_wrap(loamx_ctx* ctx, void* nccl_comm, loamx_comm** out);
void loamx_comm_destroy(loamx_comm* comm);
/* what RCCL reports for the communicator: ncclCommCount / ncclCommUserRank / ncclCommCuDevice */
int loamx_comm_info(const loamx_comm* comm, int* world_size, int* rank, int* device);
/* d_local: this rank's n_local records (device); d_all: total_pairs records (device), filled in pair-id order on
 * every rank. n_local must equal this rank's loamx_shard_range count. Asynchronous on the context's stream. */
int loamx_gather_results_dev(loamx_ctx* ctx, loamx_comm* comm, const loamx_reg_result* d_local, size_t n_local,
                             size_t total_pairs, loamx_reg_result* d_all);
/* all ranks wait for each other (1-element all-reduce + stream synchronisation); *max_value, if given, is replaced by
 * the maximum over ranks (the bench's max-over-ranks timing without a second communication library) */
int loamx_comm_barrier(loamx_ctx* ctx, loamx_comm* comm, double* max_value);
/* What the two entry points above have really enqueued on this communicator so far, by kind. A one-rank communicator
 * takes the device-copy shortcut (LOAMX_COMM_STAT_MEMCPY) unless the context's option FORCE_RCCL is set: then the
 * gather enqueues ncclAllGather AND the grouped ncclBroadcast form (in place, same bytes), the barrier ncclAllReduce —
 * the pre-flight of a box without a second GPU (tools/multi_gpu_selfcheck.py, tests/test_gpu_multi.py).
 * Environment LOAMX_RCCL_LIB names the RCCL library to dlopen instead of librccl.so.1 (a missing file: LOAMX_ERR_COMM). */
enum {
  LOAMX_COMM_STAT_ALL_GATHER = 0,
  LOAMX_COMM_STAT_BROADCAST = 1, /* members of the grouped broadcast (one per non-empty shard) */
  LOAMX_COMM_STAT_ALL_REDUCE = 2,
  LOAMX_COMM_STAT_MEMCPY = 3, /* one-rank shortcuts: no collective was enqueued */
  LOAMX_COMM_STAT_COUNT = 4
};
int loamx_comm_stats(const loamx_comm* comm, uint64_t counts[LOAMX_COMM_STAT_COUNT]);

/* ---- per-kernel timing (hipEvents on the context stream), for bench.py's roofline object ------- */
enum {
  LOAMX_K_CURVATURE = 0, /* curvature + validity, 33 B/point algorithmic */
  LOAMX_K_SELECT = 1,    /* per-sector greedy selection */
  LOAMX_K_COMPACT = 2,   /* feature gather */
  LOAMX_K_GRID = 3,      /* spatial index builds (targets: searched; sources: ordered): 24 B read + 32 B written per point,
                            + 12 B of float copies and 4 B per grid cell for the target sets that are searched by cells */
  LOAMX_K_ASSOC = 4,     /* kNN + line/plane fit */
  LOAMX_K_SWEEP = 5,     /* residual / Jacobian / normal equations, 56 B per plane + 72 B per edge slot streamed */
  LOAMX_K_LM = 6,        /* per-pair trust-region bookkeeping */
  LOAMX_K_MOMENT = 7,    /* plane moment pass (Gram matrix of the plane coefficients), 56 B per plane slot */
  LOAMX_K_KNN_PLANE = 8, /* sub-scope of LOAMX_K_ASSOC: the round-1 k-NN kernel of the plane features alone
                            (instruction-bound: bench.py prices it against the vector-issue roofline) */
  LOAMX_K_EXTRACT_FUSED = 9, /* curvature + validity + selection + compaction in one pass over the scan: 24 B/point read
                                (12 with float input) + (4 + 24) B per feature written. LOAMX_K_CURVATURE / _SELECT count
                                the separate kernels, which run when the parameters rule the fused one out */
  LOAMX_K_INFORMATION = 10, /* information_kernel + information_finish_kernel: 72 B per edge + 56 B per plane slot streamed */
  LOAMX_K_CLOUD_ACCUMULATE = 11,       /* cloud map: the accumulate kernel with run combining: 24 B/point read (12 with float input) */
  LOAMX_K_CLOUD_ACCUMULATE_PLAIN = 12, /* ... and its one-point-one-claim form (context option NO_CLOUDMAP_COMBINE) */
  LOAMX_K_CLOUD_LIST = 13,             /* cloud map: new-voxel flags, compaction and append of an add */
  LOAMX_K_CLOUD_EMIT = 14,             /* cloud map: flags, compaction and centroid scatter of an emit */
  LOAMX_K_COUNT = 15
};
typedef struct {
  uint64_t launches;
  double total_ms;
  double algorithmic_bytes; /* summed over launches */
} loamx_kernel_stat;
int loamx_ctx_enable_kernel_timing(loamx_ctx* ctx, int enable);
int loamx_ctx_reset_kernel_stats(loamx_ctx* ctx);
/* synchronises the stream, resolves pending events, fills stats[LOAMX_K_COUNT] */
int loamx_ctx_get_kernel_stats(loamx_ctx* ctx, loamx_kernel_stat* stats);
const char* loamx_kernel_name(int kernel_id);

/* ---- synthetic workload generator (tests and bench only) ------------------------- */
/* ground-truth target_T_source of pair `pair_id` */
void loamx_synth_pair_pose(uint64_t seed, uint64_t pair_id, double pose_out[7]);
/* host generation of one scan (which: 0 = target scan A, 1 = source scan B) */
void loamx_synth_scan_host(uint64_t seed, uint64_t pair_id, uint32_t which, uint32_t scan_lines,
                           uint32_t points_per_line, double sigma, double* xyz_out);
/* device generation of n_pairs x 2 scans (target first), bit-identical to the host generator */
int loamx_synth_scan_pairs_dev(loamx_ctx* ctx, uint64_t seed, uint64_t first_pair, size_t n_pairs,
                               uint32_t scan_lines, uint32_t points_per_line, double sigma, double* d_xyz);

/* raw device memory helpers so that hosts without torch can drive the _dev entry points */
int loamx_dev_alloc(loamx_ctx* ctx, size_t bytes, void** d_ptr);
int loamx_dev_free(loamx_ctx* ctx, void* d_ptr);
int loamx_copy_to_device(loamx_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int loamx_copy_to_host(loamx_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* LOAMX_H_ */
