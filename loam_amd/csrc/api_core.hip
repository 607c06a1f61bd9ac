// api_core.hip — the context of the C ABI of libloamx.so (include/loamx.h): creation, options, workspace and error helpers,
// per-kernel hipEvent timing, the non-finite input check, parameter translation, device memory helpers, the synthetic workload.
// No CPU compute path exists here: without a usable HIP device every entry point fails.
#include "api_host.h"
#include "synth.h"

using namespace loamx;

namespace loamx {
thread_local LaunchScope* g_launch_scope = nullptr;
int g_debug_sync = getenv("LOAMX_DEBUG_SYNC") ? 1 : 0;
thread_local uint32_t g_extract_route = 0;
}

namespace {

const char* kKernelNames[LOAMX_K_COUNT] = {"curvature_valid_kernel", "select_kernel", "compact_kernel",
                                           "grid_build_kernel",      "associate_kernel", "sweep_kernel",
                                           "lm_kernels",             "moment_kernel",    "knn_plane_kernel",
                                           "extract_fused_kernel",   "information_kernel", "cloud_accumulate_kernel",
                                           "cloud_accumulate_plain_kernel", "cloud_list_kernels", "cloud_emit_kernels"};

struct OptionName {
  const char* name;
  bool extract;  // bit of loamx_ctx::extract_flags, else of reg_flags
  uint32_t bit;
};
const OptionName kOptionNames[] = {
    {"FORCE_TIE_REPLAY", true, kFlagForceReplay}, {"FORCE_SCAN_GIVEUP", true, kFlagForceGiveUp}, {"CURV_V1", true, kFlagCurvV1},
    {"NO_FUSED_COMPACT", true, kFlagNoFusedCompact}, {"NO_MIS_SELECT", true, kFlagNoMisSelect}, {"FUSED_EXTRACT", true, kFlagFusedExtract},
    {"NO_ROW_SELECT", true, kFlagNoRowSelect}, {"FUSED_ROWS", true, kFlagFusedRows}, {"NO_SPLIT_CURV", true, kFlagNoSplitCurv}, {"STAGE_ALWAYS", true, kFlagStageAlways},
    {"NO_MOMENTS", false, kRegFlagNoMoments}, {"NO_PACKED_GRID", false, kRegFlagNoPackedGrid}, {"NO_BIG_GRID", false, kRegFlagNoBigGrid},
    {"NO_GRID_SIDE", false, kRegFlagNoGridSide}, {"DEBUG_POISON", false, kRegFlagPoison},
    {"QUEUE_TWO_STAGE", false, kRegFlagQueueTwoStage}, {"QUEUE_ONE_STAGE", false, kRegFlagQueueOneStage},
    {"NO_MIXED_ASSOC", false, kRegFlagNoMixedAssoc}, {"FORCE_RCCL", false, kRegFlagForceRccl},
    {"NO_COOP_LEFT", false, kRegFlagNoCoopLeft}, {"NO_COOP_ROWS", false, kRegFlagNoCoopRows}, {"NO_REF_MOMENTS", false, kRegFlagNoRefMoments},
    {"NO_EXTRACT_BOXES", false, kRegFlagNoExtractBoxes}, {"CHECK_FINITE", false, kRegFlagCheckFinite},
    {"NO_SMALL_SETS", false, kRegFlagNoSmallSets}, {"FORCE_LATE_VERIFY", false, kRegFlagForceLate},
    {"NO_LIVE_DEAL", false, kRegFlagNoLiveDeal}, {"NO_CLOUDMAP_COMBINE", false, kRegFlagNoCloudmapCombine},
    {"NO_SEGMENT_TILES", false, kRegFlagNoSegmentTiles}, {"NO_VISIBILITY_RANGES", false, kRegFlagNoVisibilityRanges},
    {"NO_OCCUPANCY_COMBINE", false, kRegFlagNoOccupancyCombine}, {"NO_SURFEL_COMBINE", false, kRegFlagNoSurfelCombine},
    {"NO_LOCALIZE_PLANES", false, kRegFlagNoLocalizePlanes}, {"NO_DISTANCE_EARLY_EXIT", false, kRegFlagNoDistanceEarlyExit},
    {"RAYCAST_COMBINE", false, kRegFlagRaycastCombine}};

}  // namespace

namespace loamx {

int fail(loamx_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->last_error = msg;
  return code;
}

int ensure(loamx_ctx* ctx, Buf& b, size_t bytes) {
  if (bytes == 0) bytes = 8;
  if (b.cap >= bytes) return LOAMX_OK;
  if (b.p) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipFree(b.p));
    b.p = nullptr, b.cap = 0;
  }
  HIP_TRY(ctx, hipMalloc(&b.p, bytes));
  b.cap = bytes;
  return LOAMX_OK;
}
int ensure(loamx_ctx* ctx, int id, size_t bytes) { return ensure(ctx, ctx->ws[id], bytes); }

// ---- non-finite input (loamx.h: "Non-finite input") -------------------------------------------------------------------
// The reference is undefined on NaN / Inf coordinates (features-inl.h:38 sorts on curvatures computed from them; nanoflann and
// Ceres receive them as they are). Host entry points refuse such input; "_dev" entry points look only when the context option
// CHECK_FINITE is set (one small kernel + a 4-byte read-back).
const char* const kNonFiniteMsg = "non-finite coordinate in the input (the reference's behaviour is undefined there)";
bool host_all_finite(const void* p, bool f32, size_t n_scalars) {
  if (!p) return true;
  if (f32) {
    const float* v = static_cast<const float*>(p);
    float acc = 0.0f;
    for (size_t i = 0; i < n_scalars; i++) acc += v[i] * 0.0f;  // 0 unless some v[i] is NaN or infinite
    return acc == 0.0f;
  }
  const double* v = static_cast<const double*>(p);
  double acc = 0.0;
  for (size_t i = 0; i < n_scalars; i++) acc += v[i] * 0.0;
  return acc == 0.0;
}

// timing helpers ------------------------------------------------------------------------------------
hipEvent_t take_event(loamx_ctx* ctx) {
  if (!ctx->event_pool.empty()) {
    hipEvent_t e = ctx->event_pool.back();
    ctx->event_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

int finite_begin(loamx_ctx* ctx) {
  ENSURE(ctx, WS_FINITE_FLAG, 16);
  untimed(ctx);
  HIP_TRY(ctx, hipMemsetAsync(ctx->ws[WS_FINITE_FLAG].p, 0, 16, ctx->stream));
  return LOAMX_OK;
}
// d_n == nullptr: `stride` points per set
void finite_add(loamx_ctx* ctx, const void* d_pts, bool f32, const uint32_t* d_n, size_t n_sets, size_t stride, uint32_t pitch) {
  if (d_pts && n_sets && stride) launch_check_finite(d_pts, f32, d_n, n_sets, stride, pitch, static_cast<uint32_t*>(ctx->ws[WS_FINITE_FLAG].p), ctx->stream);
}
int finite_end(loamx_ctx* ctx) {
  uint32_t bad = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&bad, ctx->ws[WS_FINITE_FLAG].p, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return bad ? fail(ctx, LOAMX_ERR_BAD_PARAM, kNonFiniteMsg) : LOAMX_OK;
}
int dev_check_finite(loamx_ctx* ctx, const void* d_pts, bool f32, const uint32_t* d_n, size_t n_sets, size_t stride, uint32_t pitch, bool force) {
  if ((!force && !(ctx->reg_flags & kRegFlagCheckFinite)) || !d_pts || n_sets == 0 || stride == 0) return LOAMX_OK;
  int rc = finite_begin(ctx);
  if (rc != LOAMX_OK) return rc;
  finite_add(ctx, d_pts, f32, d_n, n_sets, stride, pitch);
  return finite_end(ctx);
}

int check_finite_scalars(loamx_ctx* ctx, const double* d, size_t n) {
  int rc = finite_begin(ctx);
  if (rc != LOAMX_OK) return rc;
  launch_check_finite_scalars(d, n, static_cast<uint32_t*>(ctx->ws[WS_FINITE_FLAG].p), ctx->stream);
  return finite_end(ctx);
}

int check_launch(loamx_ctx* ctx, const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(ctx, LOAMX_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
  return LOAMX_OK;
}

// parameter translation -------------------------------------------------------------------------------
int make_extract_params(loamx_ctx* ctx, const loamx_lidar_params* lidar, const loamx_fe_params* fe, ExtractParams& P) {
  if (!lidar || !fe) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null parameter struct");
  if (fe->number_sectors == 0) return fail(ctx, LOAMX_ERR_BAD_PARAM, "number_sectors must be >= 1");
  if (fe->neighbor_points == 0)
    return fail(ctx, LOAMX_ERR_BAD_PARAM, "neighbor_points must be >= 1 (the reference reads point idx-1)");
  if (fe->neighbor_points > (uint64_t)kMaxNeighborPoints)
    return fail(ctx, LOAMX_ERR_UNSUPPORTED, "neighbor_points > 16 not supported by the kernels");
  if (lidar->points_per_line > (uint64_t)kMaxLineWidth)
    return fail(ctx, LOAMX_ERR_UNSUPPORTED, "points_per_line > 4096 not supported by the kernels");
  if (lidar->scan_lines * lidar->points_per_line > 0xFFFFFFFFull / 4)
    return fail(ctx, LOAMX_ERR_UNSUPPORTED, "scan too large for 32-bit point indices");
  if (fe->number_sectors > 65535) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "number_sectors > 65535");
  P = ExtractParams{};
  P.H = (uint32_t)lidar->scan_lines, P.W = (uint32_t)lidar->points_per_line;
  P.np = (uint32_t)fe->neighbor_points, P.S = (uint32_t)fe->number_sectors;
  P.pps = P.W / P.S;
  const uint64_t longest = (uint64_t)P.W - (uint64_t)(P.S - 1) * P.pps;  // last sector takes the remainder
  const uint64_t lim = 0x7FFFFFFFull;
  P.max_edge = (uint32_t)(fe->max_edge_feats_per_sector < lim ? fe->max_edge_feats_per_sector : lim);
  P.max_planar = (uint32_t)(fe->max_planar_feats_per_sector < lim ? fe->max_planar_feats_per_sector : lim);
  P.cap_edge = (uint32_t)((uint64_t)P.max_edge + 1 < longest ? (uint64_t)P.max_edge + 1 : longest);
  P.cap_planar = (uint32_t)((uint64_t)P.max_planar + 1 < longest ? (uint64_t)P.max_planar + 1 : longest);
  if (P.cap_edge == 0) P.cap_edge = 1;
  if (P.cap_planar == 0) P.cap_planar = 1;
  P.min_range = lidar->min_range, P.max_range = lidar->max_range;
  P.edge_thr = fe->edge_feat_threshold, P.planar_thr = fe->planar_feat_threshold;
  P.occ_thr = fe->occlusion_thresh, P.par_thr = fe->parallel_thresh;
  P.flags = ctx ? ctx->extract_flags : 0u;  // the context's switches: results never depend on them
  return LOAMX_OK;
}

int make_reg_config(loamx_ctx* ctx, const loamx_reg_params* r, RegConfig& C) {
  if (!r) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null registration params");
  if (r->num_edge_neighbors > (uint64_t)kMaxK || r->num_plane_neighbors > (uint64_t)kMaxK)
    return fail(ctx, LOAMX_ERR_UNSUPPORTED, "num_*_neighbors > 16 not supported by the kernels");
  if (r->min_plane_fit_points < 3 && r->num_plane_neighbors > 0)
    return fail(ctx, LOAMX_ERR_BAD_PARAM, "min_plane_fit_points must be >= 3");
  if (r->min_line_fit_points < 2 && r->num_edge_neighbors > 0)
    return fail(ctx, LOAMX_ERR_BAD_PARAM, "min_line_fit_points must be >= 2");
  if (r->max_iterations > 1000) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "max_iterations > 1000");
  memset(&C, 0, sizeof(C));
  auto kind_config = [](uint64_t k, double radius, uint64_t min_pts) {
    return RegKindConfig{(int)k, radius, (int)(min_pts > 64 ? 64 : min_pts), knn_radius_pass_max(radius)};
  };
  C.kind[kEdge] = kind_config(r->num_edge_neighbors, r->max_edge_neighbor_dist, r->min_line_fit_points);
  C.kind[kPlane] = kind_config(r->num_plane_neighbors, r->max_plane_neighbor_dist, r->min_plane_fit_points);
  C.min_line_cond = r->min_line_condition_number, C.max_avg_plane_dist = r->max_avg_point_plane_dist;
  C.max_iterations = (uint32_t)r->max_iterations;
  C.rot_thresh = r->rotation_convergence_thresh, C.pos_thresh = r->position_convergence_thresh;
  C.min_associations = (uint32_t)(r->min_associations > 0xFFFFFFFFull ? 0xFFFFFFFFull : r->min_associations);
  C.flags = ctx ? ctx->reg_flags : 0u;
  return LOAMX_OK;
}

int resolve_events(loamx_ctx* ctx) {
  if (ctx->pending.empty()) return LOAMX_OK;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (PendingEvent& pe : ctx->pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, pe.e0, pe.e1) == hipSuccess) {
      ctx->stats[pe.kernel].launches++;
      ctx->stats[pe.kernel].total_ms += (double)ms;
      ctx->stats[pe.kernel].algorithmic_bytes += pe.bytes;
    }
    if (pe.own_e0) ctx->event_pool.push_back(pe.e0);
    ctx->event_pool.push_back(pe.e1);
  }
  ctx->pending.clear();
  ctx->tail_fresh = false;
  return LOAMX_OK;
}

}  // namespace loamx

/* ================================================================================================== */
extern "C" {

void loamx_default_fe_params(loamx_fe_params* p) { *p = loamx_fe_params{3, 6, 10, 50, 100.0, 1.0, 0.5, 1.0}; }
void loamx_default_reg_params(loamx_reg_params* p) {
  *p = loamx_reg_params{5, 1.0, 3, 10.0, 5, 2.0, 4, 0.1, 10, 1e-3, 1e-2, 100};
}

const char* loamx_status_string(int status) {
  switch (status) {
    case LOAMX_OK: return "ok";
    case LOAMX_ERR_SCAN_SIZE: return "LOAM: provided lidar scan size does not match provided lidar parameters";
    case LOAMX_ERR_BAD_PARAM: return "bad parameter";
    case LOAMX_ERR_HIP: return "HIP error";
    case LOAMX_ERR_CAPACITY: return "output capacity too small";
    case LOAMX_ERR_UNSUPPORTED: return "unsupported parameter combination";
    case LOAMX_ERR_NO_DEVICE: return "no usable HIP device";
    case LOAMX_ERR_COMM: return "RCCL error";
    default: return "unknown status";
  }
}

const char* loamx_last_error(const loamx_ctx* ctx) { return ctx ? ctx->last_error.c_str() : ""; }
const char* loamx_kernel_name(int id) { return (id >= 0 && id < LOAMX_K_COUNT) ? kKernelNames[id] : "?"; }

int loamx_ctx_create(int device, loamx_ctx** out) {
  if (!out) return LOAMX_ERR_BAD_PARAM;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return LOAMX_ERR_NO_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return LOAMX_ERR_NO_DEVICE;
  loamx_ctx* ctx = new loamx_ctx;
  ctx->device = device;
  if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess ||
      hipHostMalloc(reinterpret_cast<void**>(&ctx->h_pinned), 256, hipHostMallocDefault) != hipSuccess) {
    delete ctx;
    return LOAMX_ERR_HIP;
  }
  ctx->stream = ctx->own_stream;
  // the switches' defaults: the environment, read here and nowhere else
  for (const OptionName& o : kOptionNames)
    if (getenv((std::string("LOAMX_") + o.name).c_str())) (o.extract ? ctx->extract_flags : ctx->reg_flags) |= o.bit;
  if (const char* mc = getenv("LOAMX_MAP_CELLS_LOG2")) ctx->map_cells_log2 = atoi(mc);
  if (const char* sc = getenv("LOAMX_STREAM_CHUNK_PAIRS")) ctx->stream_chunk_pairs = atoi(sc) > 0 ? atoi(sc) : 0;
  // optional: without the auxiliary stream the edge and plane association chains simply run in sequence
  // The auxiliary streams carry the small, latency-bound kernels next to the big ones of the main stream. Round 1 gave
  // them the highest priority (their workgroups dispatched as soon as they are ready: association 2.61 -> 2.57 ms then);
  // with the round-2 kernels it is the other way round (2.12 -> 2.09 ms at the LOWEST priority — HIP's range here is
  // least = 1, greatest = -1, the context stream runs at 0: the plane k-NN kernel is the critical path and loses less to
  // its neighbours). LOAMX_AUX_HIGH_PRIO=1 restores the old arrangement. (Round 3: priority 1 / 0 / -1 for the queue
  // chain's stream: 2.077 / 2.084 / 2.090 ms.)
  int prio_least = 0, prio_greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
  if (!getenv("LOAMX_NO_AUX_STREAM") &&
      hipStreamCreateWithPriority(&ctx->aux_stream, hipStreamNonBlocking, getenv("LOAMX_AUX_HIGH_PRIO") ? prio_greatest : prio_least) == hipSuccess) {
    if (hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_mid, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming) != hipSuccess) {
      (void)hipStreamDestroy(ctx->aux_stream);
      ctx->aux_stream = nullptr;
    } else if (!getenv("LOAMX_NO_AUX2_STREAM") &&
               hipStreamCreateWithPriority(&ctx->aux2_stream, hipStreamNonBlocking, (getenv("LOAMX_AUX_HIGH_PRIO") || getenv("LOAMX_AUX2_HIGH_PRIO")) ? prio_greatest : prio_least) == hipSuccess) {
      if (hipEventCreateWithFlags(&ctx->ev_join2, hipEventDisableTiming) != hipSuccess) {
        (void)hipStreamDestroy(ctx->aux2_stream);
        ctx->aux2_stream = nullptr;
      }
    }
  }
  *out = ctx;
  return LOAMX_OK;
}

void loamx_ctx_destroy(loamx_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  for (PendingEvent& pe : ctx->pending) {
    if (pe.own_e0) (void)hipEventDestroy(pe.e0);
    (void)hipEventDestroy(pe.e1);
  }
  for (hipEvent_t e : ctx->event_pool) (void)hipEventDestroy(e);
  for (Buf& b : ctx->ws)
    if (b.p) (void)hipFree(b.p);
  for (Buf(&bk)[2] : ctx->wsk)
    for (Buf& b : bk)
      if (b.p) (void)hipFree(b.p);
  if (ctx->h_pinned) (void)hipHostFree(ctx->h_pinned);
  if (ctx->aux_stream) {
    (void)hipStreamSynchronize(ctx->aux_stream);
    (void)hipStreamDestroy(ctx->aux_stream);
  }
  if (ctx->aux2_stream) {
    (void)hipStreamSynchronize(ctx->aux2_stream);
    (void)hipStreamDestroy(ctx->aux2_stream);
  }
  if (ctx->copy_stream) {
    (void)hipStreamSynchronize(ctx->copy_stream);
    (void)hipStreamDestroy(ctx->copy_stream);
  }
  for (int b = 0; b < 2; b++) {
    if (ctx->ev_up[b]) (void)hipEventDestroy(ctx->ev_up[b]);
    if (ctx->ev_free[b]) (void)hipEventDestroy(ctx->ev_free[b]);
  }
  if (ctx->ev_join2) (void)hipEventDestroy(ctx->ev_join2);
  if (ctx->ev_counts) (void)hipEventDestroy(ctx->ev_counts);
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
  if (ctx->ev_mid) (void)hipEventDestroy(ctx->ev_mid);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
  delete ctx;
}

int loamx_ctx_set_stream(loamx_ctx* ctx, void* hip_stream) {
  API_LOCK(ctx);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx->own_stream;
  return LOAMX_OK;
}

int loamx_ctx_synchronize(loamx_ctx* ctx) {
  API_ENTER(ctx);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LOAMX_OK;
}

int loamx_ctx_set_option(loamx_ctx* ctx, const char* name, int value) {
  if (!ctx || !name) return LOAMX_ERR_BAD_PARAM;
  API_LOCK(ctx);
  if (!strcmp(name, "MAP_CELLS_LOG2")) {
    ctx->map_cells_log2 = value;
    return LOAMX_OK;
  }
  if (!strcmp(name, "STREAM_CHUNK_PAIRS")) {
    if (value < 0) return fail(ctx, LOAMX_ERR_BAD_PARAM, "STREAM_CHUNK_PAIRS: a number of pairs (0 = default)");
    ctx->stream_chunk_pairs = value;
    return LOAMX_OK;
  }
  for (const OptionName& o : kOptionNames)
    if (!strcmp(name, o.name)) {
      uint32_t& w = o.extract ? ctx->extract_flags : ctx->reg_flags;
      w = value ? (w | o.bit) : (w & ~o.bit);
      return LOAMX_OK;
    }
  return fail(ctx, LOAMX_ERR_BAD_PARAM, std::string("unknown option ") + name);
}

int loamx_ctx_get_option(loamx_ctx* ctx, const char* name, int* value) {
  if (!ctx || !name || !value) return LOAMX_ERR_BAD_PARAM;
  API_LOCK(ctx);
  if (!strcmp(name, "MAP_CELLS_LOG2")) {
    *value = ctx->map_cells_log2;
    return LOAMX_OK;
  }
  if (!strcmp(name, "STREAM_CHUNK_PAIRS")) {
    *value = ctx->stream_chunk_pairs;
    return LOAMX_OK;
  }
  for (const OptionName& o : kOptionNames)
    if (!strcmp(name, o.name)) {
      *value = ((o.extract ? ctx->extract_flags : ctx->reg_flags) & o.bit) ? 1 : 0;
      return LOAMX_OK;
    }
  return fail(ctx, LOAMX_ERR_BAD_PARAM, std::string("unknown option ") + name);
}

int loamx_ctx_extract_counters(loamx_ctx* ctx, uint64_t* tie_replays, uint64_t* scan_fallbacks) {
  API_ENTER(ctx);
  unsigned long long ev[2] = {0, 0};
  if (ctx->ws[WS_EXTRACT_EVENTS].p) {
    HIP_TRY(ctx, hipMemcpyAsync(ev, ctx->ws[WS_EXTRACT_EVENTS].p, sizeof(ev), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (tie_replays) *tie_replays = ev[0];
  if (scan_fallbacks) *scan_fallbacks = ev[1];
  return LOAMX_OK;
}

int loamx_ctx_last_extract_route(loamx_ctx* ctx, uint32_t* bits) {
  if (!ctx || !bits) return LOAMX_ERR_BAD_PARAM;
  API_LOCK(ctx);
  *bits = ctx->last_extract_route;
  return LOAMX_OK;
}

size_t loamx_edge_capacity(const loamx_lidar_params* lidar, const loamx_fe_params* fe) {
  ExtractParams P;
  if (make_extract_params(nullptr, lidar, fe, P) != LOAMX_OK) return 0;
  return edge_capacity(P);
}
size_t loamx_planar_capacity(const loamx_lidar_params* lidar, const loamx_fe_params* fe) {
  ExtractParams P;
  if (make_extract_params(nullptr, lidar, fe, P) != LOAMX_OK) return 0;
  return planar_capacity(P);
}

/* ---- kernel timing ------------------------------------------------------------------------------------ */
int loamx_ctx_enable_kernel_timing(loamx_ctx* ctx, int enable) {
  API_LOCK(ctx);
  ctx->timing = enable != 0;
  return LOAMX_OK;
}

static int read_sweep_slots(loamx_ctx* ctx, unsigned long long out[6]) {
  out[0] = out[1] = out[2] = out[3] = out[4] = out[5] = 0;
  if (!ctx->ws[WS_COUNTERS].p) return LOAMX_OK;
  HIP_TRY(ctx, hipMemcpy(out, wsp<unsigned char>(ctx, WS_COUNTERS) + 8, 48, hipMemcpyDeviceToHost));
  return LOAMX_OK;
}

int loamx_ctx_reset_kernel_stats(loamx_ctx* ctx) {
  API_ENTER(ctx);
  int rc = resolve_events(ctx);
  if (rc != LOAMX_OK) return rc;
  memset(ctx->stats, 0, sizeof(ctx->stats));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->ws[WS_COUNTERS].p) HIP_TRY(ctx, hipMemset(wsp<unsigned char>(ctx, WS_COUNTERS) + 8, 0, 48));
  if (ctx->ws[WS_EXTRACT_EVENTS].p) {
    unsigned long long ev[4] = {0, 0, 0, 0};
    HIP_TRY(ctx, hipMemcpy(ev, ctx->ws[WS_EXTRACT_EVENTS].p, sizeof(ev), hipMemcpyDeviceToHost));
    ctx->features_base = ev[2];
  }
  return LOAMX_OK;
}

int loamx_ctx_get_kernel_stats(loamx_ctx* ctx, loamx_kernel_stat* stats) {
  if (!ctx || !stats) return LOAMX_ERR_BAD_PARAM;
  API_ENTER(ctx);
  int rc = resolve_events(ctx);
  if (rc != LOAMX_OK) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  unsigned long long slots[6];
  rc = read_sweep_slots(ctx, slots);
  if (rc != LOAMX_OK) return rc;
  memcpy(stats, ctx->stats, sizeof(ctx->stats));
  // sweep: one association record per slot (edge 72 B, plane 56 B)
  stats[LOAMX_K_SWEEP].algorithmic_bytes = 72.0 * (double)slots[0] + 56.0 * (double)slots[1];
  // associate: read the 24 B source point, write the record + the 4 B nearest index
  stats[LOAMX_K_ASSOC].algorithmic_bytes = 100.0 * (double)slots[2] + 84.0 * (double)slots[3];
  stats[LOAMX_K_MOMENT].algorithmic_bytes = 56.0 * (double)slots[4];  // moment pass: every plane record once
  stats[LOAMX_K_GRID].algorithmic_bytes = (double)slots[5];            // index builds: counted by the build kernels
  if (ctx->ws[WS_EXTRACT_EVENTS].p) {  // fused extraction: + (4 + 24) B per feature written (counted by the kernel since the reset)
    unsigned long long ev[4] = {0, 0, 0, 0};
    HIP_TRY(ctx, hipMemcpy(ev, ctx->ws[WS_EXTRACT_EVENTS].p, sizeof(ev), hipMemcpyDeviceToHost));
    stats[LOAMX_K_EXTRACT_FUSED].algorithmic_bytes += 28.0 * (double)(ev[2] - ctx->features_base);
    // the selection with its fused compaction copies every feature: 24 B read + 24 B written per feature on top of the
    // curvature words it was priced with at launch (without them the scope read as 0.07 of HBM while the
    // kernel moves 4.9 TB/s); the features are counted by the kernel itself (events[2])
    if (stats[LOAMX_K_SELECT].launches != 0 && stats[LOAMX_K_EXTRACT_FUSED].launches == 0)
      stats[LOAMX_K_SELECT].algorithmic_bytes += 48.0 * (double)(ev[2] - ctx->features_base);
  }
  return LOAMX_OK;
}

/* ---- synthetic workload ------------------------------------------------------------------------------- */
void loamx_synth_pair_pose(uint64_t seed, uint64_t pair_id, double pose_out[7]) {
  const loamx_synth::Pose7 p = loamx_synth::pair_pose(seed, pair_id);
  for (int i = 0; i < 4; i++) pose_out[i] = p.q[i];
  for (int i = 0; i < 3; i++) pose_out[4 + i] = p.t[i];
}

void loamx_synth_scan_host(uint64_t seed, uint64_t pair_id, uint32_t which, uint32_t H, uint32_t W, double sigma,
                           double* xyz_out) {
  const loamx_synth::Pose7 pose = loamx_synth::pair_pose(seed, pair_id);
  for (uint32_t l = 0; l < H; l++)
    for (uint32_t c = 0; c < W; c++)
      loamx_synth::scan_point(seed, pair_id, which, pose, l, c, H, W, sigma, xyz_out + 3 * ((size_t)l * W + c));
}

int loamx_synth_scan_pairs_dev(loamx_ctx* ctx, uint64_t seed, uint64_t first_pair, size_t n_pairs, uint32_t H, uint32_t W,
                               double sigma, double* d_xyz) {
  API_ENTER(ctx);
  launch_synth_pairs(seed, first_pair, n_pairs, H, W, sigma, d_xyz, ctx->stream);
  CHECK_LAUNCH(ctx, "synth_kernel");
  return LOAMX_OK;
}

/* ---- raw device memory helpers ------------------------------------------------------------------------ */
int loamx_dev_alloc(loamx_ctx* ctx, size_t bytes, void** d_ptr) {
  if (!ctx || !d_ptr) return LOAMX_ERR_BAD_PARAM;
  API_ENTER(ctx);
  HIP_TRY(ctx, hipMalloc(d_ptr, bytes ? bytes : 8));
  return LOAMX_OK;
}
int loamx_dev_free(loamx_ctx* ctx, void* d_ptr) {
  API_ENTER(ctx);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipFree(d_ptr));
  return LOAMX_OK;
}
int loamx_copy_to_device(loamx_ctx* ctx, void* d_dst, const void* h_src, size_t bytes) {
  API_ENTER(ctx);
  HIP_TRY(ctx, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LOAMX_OK;
}
int loamx_copy_to_host(loamx_ctx* ctx, void* h_dst, const void* d_src, size_t bytes) {
  API_ENTER(ctx);
  HIP_TRY(ctx, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LOAMX_OK;
}

}  // extern "C"
