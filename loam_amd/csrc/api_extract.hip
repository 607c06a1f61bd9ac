// api_extract.hip — feature extraction: the driver over device-resident scans (extract_dev) and the entry points around it.
#include "api_host.h"

using namespace loamx;

namespace loamx {

// extraction over device-resident scans ------------------------------------------------------------------
// d_xyz: double, or float when f32 (FP32-input path)
int extract_dev(loamx_ctx* ctx, const void* d_xyz, bool f32, size_t n_scans, const ExtractParams& P, uint32_t* d_edge_idx,
                uint32_t* d_n_edge, double* d_edge_xyz, uint32_t* d_planar_idx, uint32_t* d_n_planar,
                double* d_planar_xyz, bool only_curvature_mask, ExtractBoxes* boxes) {
  const size_t N = (size_t)P.H * P.W;
  if (boxes) *boxes = ExtractBoxes{};
  // the launchers note their choices in g_extract_route; whichever way this call returns, the context keeps them
  struct RouteKeeper {
    loamx_ctx* c;
    explicit RouteKeeper(loamx_ctx* c_) : c(c_) { g_extract_route = 0; }
    ~RouteKeeper() { c->last_extract_route = g_extract_route; }
  } route_keeper(ctx);
  if (n_scans == 0) return LOAMX_OK;
  untimed(ctx);
  if (N == 0) {
    if (!only_curvature_mask) {
      untimed(ctx);
      HIP_TRY(ctx, hipMemsetAsync(d_n_edge, 0, n_scans * sizeof(uint32_t), ctx->stream));
      HIP_TRY(ctx, hipMemsetAsync(d_n_planar, 0, n_scans * sizeof(uint32_t), ctx->stream));
    }
    return LOAMX_OK;
  }
  ENSURE(ctx, WS_CURV, n_scans * N * sizeof(double));
  ENSURE(ctx, WS_MASK, n_scans * N);
  if (only_curvature_mask) {  // loamx_compute_curvature / loamx_compute_valid_points: the standalone kernel
    {
      TimedScope t(ctx, LOAMX_K_CURVATURE, (double)n_scans * (double)N * (f32 ? 21.0 : 33.0), true);
      launch_curvature_valid(d_xyz, f32, n_scans, P, wsp<double>(ctx, WS_CURV), wsp<uint8_t>(ctx, WS_MASK), ctx->stream);
    }
    CHECK_LAUNCH(ctx, "curvature_valid_kernel");
    return LOAMX_OK;
  }
  const size_t groups = n_scans * P.H * P.S;
  ENSURE(ctx, ctx->wsk[WSK_STAGE][kEdge], groups * P.cap_edge * sizeof(uint32_t));
  ENSURE(ctx, ctx->wsk[WSK_STAGE][kPlane], groups * P.cap_planar * sizeof(uint32_t));
  ENSURE(ctx, ctx->wsk[WSK_CNT][kEdge], groups * sizeof(uint32_t));
  ENSURE(ctx, ctx->wsk[WSK_CNT][kPlane], groups * sizeof(uint32_t));
  ExtractStage st{wskp<uint32_t>(ctx, WSK_STAGE, kEdge), wskp<uint32_t>(ctx, WSK_STAGE, kPlane),
                  wskp<uint32_t>(ctx, WSK_CNT, kEdge), wskp<uint32_t>(ctx, WSK_CNT, kPlane)};
  // the selection writes the final feature arrays itself when it can (launch_select); its chained scan over the
  // lines of a scan needs the per-line slots zeroed
  // ... and one more word behind them: the give-up flag of that chained scan (zeroed by the same memset)
  const size_t n_lines = n_scans * P.H;
  ENSURE(ctx, WS_LINE_TOT, (n_lines + 1) * sizeof(unsigned long long));
  {
    const bool fresh = ctx->ws[WS_EXTRACT_EVENTS].cap == 0;  // cumulative counters: zeroed once
    ENSURE(ctx, WS_EXTRACT_EVENTS, 4 * sizeof(unsigned long long));
    untimed(ctx);
    if (fresh) HIP_TRY(ctx, hipMemsetAsync(ctx->ws[WS_EXTRACT_EVENTS].p, 0, 4 * sizeof(unsigned long long), ctx->stream));
  }
  untimed(ctx);
  uint32_t* d_gave_up = reinterpret_cast<uint32_t*>(wsp<unsigned long long>(ctx, WS_LINE_TOT) + n_lines);
  unsigned long long* d_events = wsp<unsigned long long>(ctx, WS_EXTRACT_EVENTS);
  ExtractFused fz{wsp<unsigned long long>(ctx, WS_LINE_TOT), 0u, d_xyz, f32 ? 1u : 0u, d_edge_idx, d_n_edge, d_edge_xyz,
                  edge_capacity(P), d_planar_idx, d_n_planar, d_planar_xyz, planar_capacity(P), d_gave_up, d_events, nullptr, nullptr};
  if (boxes && d_edge_xyz && d_planar_xyz && launch_select_takes_boxes(P)) {
    ENSURE(ctx, WS_BOX, 2 * n_scans * 6 * sizeof(unsigned long long));
    fz.box_min = wsp<unsigned long long>(ctx, WS_BOX), fz.box_max = fz.box_min + n_scans * 6;
  }
  untimed(ctx);
  launch_extract_init(fz.line_tot, n_lines + 1, fz.box_min, fz.box_max, fz.box_min ? n_scans * 6 : 0, ctx->stream);
  CHECK_LAUNCH(ctx, "extract_init_kernel");
  {
    // rows a5-a10 in one pass over the scan — opt-in (context option FUSED_EXTRACT; the two kernels below are the default,
    // see launch_extract_fused) and only where the parameters allow: 24 B/point read + (4 + 24) B per feature written;
    // the features are counted on the device (events[2]) for the roofline figure
    TimedScope t(ctx, LOAMX_K_EXTRACT_FUSED, (double)n_scans * (double)N * (f32 ? 12.0 : 24.0), true);
    if (launch_extract_fused(d_xyz, f32, n_scans, P, st, fz, wsp<double>(ctx, WS_CURV), wsp<uint8_t>(ctx, WS_MASK), ctx->stream)) {
      launch_replay(wsp<double>(ctx, WS_CURV), wsp<uint8_t>(ctx, WS_MASK), n_scans, P, st, fz, ctx->stream);
      launch_compact(d_xyz, f32, n_scans, P, st, d_edge_idx, d_n_edge, d_edge_xyz, edge_capacity(P), d_planar_idx, d_n_planar,
                     d_planar_xyz, planar_capacity(P), ctx->stream, d_gave_up, d_events + 1);
      g_extract_route |= LOAMX_ROUTE_FUSED_COMPACT;
      return check_launch(ctx, "extract_fused_kernel");
    }
  }
  {
    // rows a5-a10 in one kernel, four scan lines per wavefront (round 5; select_rows.h) — opt-in (context option FUSED_ROWS):
    // bit-identical, but measured slower than the two kernels (EXPERIMENTS.md round 5)
    TimedScope t(ctx, LOAMX_K_EXTRACT_FUSED, (double)n_scans * (double)N * (f32 ? 12.0 : 24.0), true);
    if (launch_extract_rows_fused(d_xyz, f32, n_scans, P, st, fz, wsp<double>(ctx, WS_CURV), wsp<uint8_t>(ctx, WS_MASK), ctx->stream)) {
      const bool fused_compact = P.S <= 64 && !(P.flags & kFlagNoFusedCompact);
      launch_replay(wsp<double>(ctx, WS_CURV), wsp<uint8_t>(ctx, WS_MASK), n_scans, P, st, fz, ctx->stream);
      launch_compact(d_xyz, f32, n_scans, P, st, d_edge_idx, d_n_edge, d_edge_xyz, edge_capacity(P), d_planar_idx, d_n_planar,
                     d_planar_xyz, planar_capacity(P), ctx->stream, fused_compact ? d_gave_up : nullptr, fused_compact ? d_events + 1 : nullptr);
      g_extract_route |= fused_compact ? LOAMX_ROUTE_FUSED_COMPACT : LOAMX_ROUTE_COMPACT;
      return check_launch(ctx, "select_rows_kernel (fused)");
    }
  }
  // Round 5: between these two kernels the curvature travels as hi words | lo words with the validity in the sign bit where
  // both know that form (kFlagSplitCurv; the selection then reads 4 instead of 9 bytes per point)
  ExtractParams Pk = P;
  if (launch_extract_split_ok(P, n_scans)) Pk.flags |= kFlagSplitCurv, g_extract_route |= LOAMX_ROUTE_SPLIT_CURV;
  const bool split = (Pk.flags & kFlagSplitCurv) != 0u;
  {
    TimedScope t(ctx, LOAMX_K_CURVATURE, (double)n_scans * (double)N * ((f32 ? 21.0 : 33.0) - (split ? 1.0 : 0.0)), true);
    launch_curvature_valid(d_xyz, f32, n_scans, Pk, wsp<double>(ctx, WS_CURV), wsp<uint8_t>(ctx, WS_MASK), ctx->stream);
  }
  CHECK_LAUNCH(ctx, "curvature_valid_kernel");
  bool fused = false, rows_ran = false;
  {
    TimedScope t(ctx, LOAMX_K_SELECT, (double)n_scans * (double)N * (split ? 4.0 : 9.0), true);
    fused = launch_select(wsp<double>(ctx, WS_CURV), wsp<uint8_t>(ctx, WS_MASK), n_scans, Pk, st, &fz, ctx->stream, &rows_ran);
    // scan lines on which a curvature tie can decide something: again, in the reference's std::sort order (a no-op without)
    launch_replay(wsp<double>(ctx, WS_CURV), wsp<uint8_t>(ctx, WS_MASK), n_scans, Pk, st, fz, ctx->stream);
    // A scan line whose wavefront gave up waiting for the lines before it (bounded wait: unusual scheduling) left its
    // features in the stage arrays; this launch then gathers the batch from them and is a no-op otherwise (every
    // workgroup reads the flag and leaves): the call stays asynchronous and never fails for that reason.
    if (fused) {
      launch_compact(d_xyz, f32, n_scans, P, st, d_edge_idx, d_n_edge, d_edge_xyz, edge_capacity(P), d_planar_idx, d_n_planar,
                     d_planar_xyz, planar_capacity(P), ctx->stream, d_gave_up, d_events + 1);
      g_extract_route |= LOAMX_ROUTE_FUSED_COMPACT;
    }
  }
  CHECK_LAUNCH(ctx, "select_kernel");
  // (the split curvature form is understood by select_rows_kernel alone: had launch_select refused it on a condition
  // launch_extract_split_ok does not share, the other selection kernels would have read hi / lo words as doubles)
  if (split && !rows_ran) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "internal: split curvature form without the row selection");
  if (fused && rows_ran && boxes && fz.box_min)
    boxes->min = fz.box_min, boxes->max = fz.box_max, boxes->bad = d_gave_up, g_extract_route |= LOAMX_ROUTE_BOXES;
  if (fused) return LOAMX_OK;
  {
    TimedScope t(ctx, LOAMX_K_COMPACT, 0.0, true);
    launch_compact(d_xyz, f32, n_scans, P, st, d_edge_idx, d_n_edge, d_edge_xyz, edge_capacity(P), d_planar_idx,
                   d_n_planar, d_planar_xyz, planar_capacity(P), ctx->stream);
    g_extract_route |= LOAMX_ROUTE_COMPACT;
  }
  CHECK_LAUNCH(ctx, "compact_kernel");
  return LOAMX_OK;
}

}  // namespace loamx

extern "C" {

/* ---- host entry points ---------------------------------------------------------------------------- */
static int host_curv_mask(loamx_ctx* ctx, const void* xyz, bool f32, size_t n_points, const loamx_lidar_params* lidar,
                          const loamx_fe_params* fe, double* curvature_out, uint8_t* mask_out) {
  API_ENTER(ctx);
  if (!lidar || !fe) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null parameter struct");
  if (n_points != lidar->scan_lines * lidar->points_per_line) {  // common.h:104-113
    char msg[256];
    snprintf(msg, sizeof(msg), "LOAM: provided lidar scan size ( %zu)  does not match provided lidar parameters (%llu x %llu)",
             n_points, (unsigned long long)lidar->scan_lines, (unsigned long long)lidar->points_per_line);
    return fail(ctx, LOAMX_ERR_SCAN_SIZE, msg);
  }
  if (n_points == 0) return LOAMX_OK;
  ExtractParams P;
  int rc = make_extract_params(ctx, lidar, fe, P);
  if (rc != LOAMX_OK) return rc;
  if (!xyz) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  const size_t scalar = f32 ? sizeof(float) : sizeof(double);
  ENSURE(ctx, WS_XYZ, n_points * 3 * scalar);
  HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[WS_XYZ].p, xyz, n_points * 3 * scalar, hipMemcpyHostToDevice, ctx->stream));
  rc = dev_check_finite(ctx, ctx->ws[WS_XYZ].p, f32, nullptr, 1, n_points, 1, true);
  if (rc != LOAMX_OK) return rc;
  rc = extract_dev(ctx, ctx->ws[WS_XYZ].p, f32, 1, P, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, true);
  if (rc != LOAMX_OK) return rc;
  if (curvature_out)
    HIP_TRY(ctx, hipMemcpyAsync(curvature_out, ctx->ws[WS_CURV].p, n_points * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (mask_out)
    HIP_TRY(ctx, hipMemcpyAsync(mask_out, ctx->ws[WS_MASK].p, n_points, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LOAMX_OK;
}

int loamx_compute_curvature(loamx_ctx* ctx, const double* xyz, size_t n_points, const loamx_lidar_params* lidar,
                            const loamx_fe_params* fe, double* curvature_out) {
  return host_curv_mask(ctx, xyz, false, n_points, lidar, fe, curvature_out, nullptr);
}

int loamx_compute_valid_points(loamx_ctx* ctx, const double* xyz, size_t n_points, const loamx_lidar_params* lidar,
                               const loamx_fe_params* fe, uint8_t* mask_out) {
  return host_curv_mask(ctx, xyz, false, n_points, lidar, fe, nullptr, mask_out);
}

int loamx_compute_curvature_f32(loamx_ctx* ctx, const float* xyz, size_t n_points, const loamx_lidar_params* lidar,
                                const loamx_fe_params* fe, double* curvature_out) {
  return host_curv_mask(ctx, xyz, true, n_points, lidar, fe, curvature_out, nullptr);
}

int loamx_compute_valid_points_f32(loamx_ctx* ctx, const float* xyz, size_t n_points, const loamx_lidar_params* lidar,
                                   const loamx_fe_params* fe, uint8_t* mask_out) {
  return host_curv_mask(ctx, xyz, true, n_points, lidar, fe, nullptr, mask_out);
}

static int host_extract(loamx_ctx* ctx, const void* xyz, bool f32, size_t n_points, const loamx_lidar_params* lidar,
                        const loamx_fe_params* fe, uint32_t* edge_idx, size_t edge_cap, size_t* n_edge,
                        uint32_t* planar_idx, size_t planar_cap, size_t* n_planar) {
  API_ENTER(ctx);
  if (!lidar || !fe || !n_edge || !n_planar) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  if (n_points != lidar->scan_lines * lidar->points_per_line) {
    char msg[256];
    snprintf(msg, sizeof(msg), "LOAM: provided lidar scan size ( %zu)  does not match provided lidar parameters (%llu x %llu)",
             n_points, (unsigned long long)lidar->scan_lines, (unsigned long long)lidar->points_per_line);
    return fail(ctx, LOAMX_ERR_SCAN_SIZE, msg);
  }
  *n_edge = 0, *n_planar = 0;
  if (n_points == 0) return LOAMX_OK;
  ExtractParams P;
  int rc = make_extract_params(ctx, lidar, fe, P);
  if (rc != LOAMX_OK) return rc;
  const size_t ecap = edge_capacity(P), pcap = planar_capacity(P);
  const size_t scalar = f32 ? sizeof(float) : sizeof(double);
  if (!xyz) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  ENSURE(ctx, WS_XYZ, n_points * 3 * scalar);
  ENSURE(ctx, ctx->wsk[WSK_IDX][kEdge], ecap * sizeof(uint32_t));
  ENSURE(ctx, ctx->wsk[WSK_IDX][kPlane], pcap * sizeof(uint32_t));
  for (int k = 0; k < 2; k++) ENSURE(ctx, ctx->wsk[WSK_N][k], sizeof(uint32_t));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[WS_XYZ].p, xyz, n_points * 3 * scalar, hipMemcpyHostToDevice, ctx->stream));
  rc = dev_check_finite(ctx, ctx->ws[WS_XYZ].p, f32, nullptr, 1, n_points, 1, true);
  if (rc != LOAMX_OK) return rc;
  rc = extract_dev(ctx, ctx->ws[WS_XYZ].p, f32, 1, P, wskp<uint32_t>(ctx, WSK_IDX, kEdge), wskp<uint32_t>(ctx, WSK_N, kEdge), nullptr,
                   wskp<uint32_t>(ctx, WSK_IDX, kPlane), wskp<uint32_t>(ctx, WSK_N, kPlane), nullptr, false);
  if (rc != LOAMX_OK) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(&ctx->h_pinned[0], ctx->wsk[WSK_N][kEdge].p, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(&ctx->h_pinned[1], ctx->wsk[WSK_N][kPlane].p, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  const size_t ne = ctx->h_pinned[0], npl = ctx->h_pinned[1];
  *n_edge = ne, *n_planar = npl;
  if (ne > edge_cap || npl > planar_cap) return fail(ctx, LOAMX_ERR_CAPACITY, "feature index capacity too small");
  if (ne) HIP_TRY(ctx, hipMemcpy(edge_idx, ctx->wsk[WSK_IDX][kEdge].p, ne * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (npl) HIP_TRY(ctx, hipMemcpy(planar_idx, ctx->wsk[WSK_IDX][kPlane].p, npl * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return LOAMX_OK;
}

int loamx_extract_features(loamx_ctx* ctx, const double* xyz, size_t n_points, const loamx_lidar_params* lidar,
                           const loamx_fe_params* fe, uint32_t* edge_idx, size_t edge_cap, size_t* n_edge,
                           uint32_t* planar_idx, size_t planar_cap, size_t* n_planar) {
  return host_extract(ctx, xyz, false, n_points, lidar, fe, edge_idx, edge_cap, n_edge, planar_idx, planar_cap, n_planar);
}

int loamx_extract_features_f32(loamx_ctx* ctx, const float* xyz, size_t n_points, const loamx_lidar_params* lidar,
                               const loamx_fe_params* fe, uint32_t* edge_idx, size_t edge_cap, size_t* n_edge,
                               uint32_t* planar_idx, size_t planar_cap, size_t* n_planar) {
  return host_extract(ctx, xyz, true, n_points, lidar, fe, edge_idx, edge_cap, n_edge, planar_idx, planar_cap, n_planar);
}

/* ---- device-resident batch entry points ----------------------------------------------------------- */
static int extract_batch_dev(loamx_ctx* ctx, const void* d_xyz, bool f32, size_t n_scans, const loamx_lidar_params* lidar,
                             const loamx_fe_params* fe, uint32_t* d_edge_idx, uint32_t* d_n_edge, double* d_edge_xyz,
                             uint32_t* d_planar_idx, uint32_t* d_n_planar, double* d_planar_xyz) {
  API_ENTER(ctx);
  ExtractParams P;
  int rc = make_extract_params(ctx, lidar, fe, P);
  if (rc != LOAMX_OK) return rc;
  rc = dev_check_finite(ctx, d_xyz, f32, nullptr, n_scans, (size_t)P.H * P.W, 1);
  if (rc != LOAMX_OK) return rc;
  return extract_dev(ctx, d_xyz, f32, n_scans, P, d_edge_idx, d_n_edge, d_edge_xyz, d_planar_idx, d_n_planar, d_planar_xyz, false);
}

int loamx_extract_features_batch_dev(loamx_ctx* ctx, const double* d_xyz, size_t n_scans, const loamx_lidar_params* lidar,
                                     const loamx_fe_params* fe, uint32_t* d_edge_idx, uint32_t* d_n_edge,
                                     double* d_edge_xyz, uint32_t* d_planar_idx, uint32_t* d_n_planar,
                                     double* d_planar_xyz) {
  return extract_batch_dev(ctx, d_xyz, false, n_scans, lidar, fe, d_edge_idx, d_n_edge, d_edge_xyz, d_planar_idx, d_n_planar, d_planar_xyz);
}

int loamx_extract_features_batch_dev_f32(loamx_ctx* ctx, const float* d_xyz, size_t n_scans, const loamx_lidar_params* lidar,
                                         const loamx_fe_params* fe, uint32_t* d_edge_idx, uint32_t* d_n_edge,
                                         double* d_edge_xyz, uint32_t* d_planar_idx, uint32_t* d_n_planar,
                                         double* d_planar_xyz) {
  return extract_batch_dev(ctx, d_xyz, true, n_scans, lidar, fe, d_edge_idx, d_n_edge, d_edge_xyz, d_planar_idx, d_n_planar, d_planar_xyz);
}

}  // extern "C"
