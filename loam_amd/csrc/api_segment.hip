// api_segment.hip — scan segmentation (loamx.h, "scan segmentation"): parameter translation with the two host-computed constants,
// the device-resident batch entry points, the one-scan host forms and the census of the last call.
#include "api_host.h"

using namespace loamx;

namespace {

// the angle checks and the two constants (FP64, libm, once per call); why: the refusal's message
int segment_constants(const loamx_segment_params* p, double out[2], const char** why) {
  if (!p) return *why = "null segment params", LOAMX_ERR_BAD_PARAM;
  if (!isfinite(p->ground_angle) || !isfinite(p->segment_angle)) return *why = "a segmentation angle is not finite", LOAMX_ERR_BAD_PARAM;
  if (!(p->ground_angle >= 0.0 && p->ground_angle < M_PI / 2)) return *why = "ground_angle outside [0, pi/2)", LOAMX_ERR_BAD_PARAM;
  if (!(p->segment_angle > 0.0 && p->segment_angle < M_PI / 2)) return *why = "segment_angle outside (0, pi/2)", LOAMX_ERR_BAD_PARAM;
  const double tg = tan(p->ground_angle), cs = cos(p->segment_angle);
  out[0] = tg * tg, out[1] = cs * cs;
  return LOAMX_OK;
}

inline uint32_t clamp32(uint64_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }

int make_segment_params(loamx_ctx* ctx, const loamx_lidar_params* lidar, const loamx_segment_params* p, size_t n_scans, SegParams& P) {
  if (!lidar || !p) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null parameter struct");
  double k[2];
  const char* why = "";
  int rc = segment_constants(p, k, &why);
  if (rc != LOAMX_OK) return fail(ctx, rc, why);
  if (lidar->scan_lines == 0 || lidar->points_per_line == 0) return fail(ctx, LOAMX_ERR_BAD_PARAM, "scan_lines and points_per_line must be >= 1");
  const double mr2 = lidar->max_range * lidar->max_range;
  if (!isfinite(mr2 * mr2)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "max_range to the fourth power is not finite");
  // (the limits make_extract_params applies to a lidar shape: whatever is segmented here can be extracted)
  if (lidar->points_per_line > (uint64_t)kMaxLineWidth) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "points_per_line > 4096 not supported by the kernels");
  if (lidar->scan_lines > 0xFFFFFFFFull || lidar->scan_lines * lidar->points_per_line > 0xFFFFFFFFull / 4)
    return fail(ctx, LOAMX_ERR_UNSUPPORTED, "scan too large for 32-bit point indices");
  if (n_scans > kSegMaxScans) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "more than 65535 scans in one segmentation call");
  P = SegParams{};
  P.H = (uint32_t)lidar->scan_lines, P.W = (uint32_t)lidar->points_per_line;
  P.G = p->ground_lines == 0 || p->ground_lines > P.H ? P.H : (uint32_t)p->ground_lines;
  P.min_range = lidar->min_range, P.max_range = lidar->max_range;
  P.tg2 = k[0], P.c2 = k[1];
  P.min_cluster = clamp32(p->min_cluster_points), P.min_tall_points = clamp32(p->min_tall_cluster_points);
  P.min_tall_lines = clamp32(p->min_tall_cluster_lines);
  P.drop_outliers = p->drop_outliers ? 1u : 0u, P.drop_ground = p->drop_ground ? 1u : 0u;
  return LOAMX_OK;
}

inline size_t round16(size_t v) { return (v + 15) & ~(size_t)15; }

// the scans of the call (the caller holds ctx->mu, has selected the device and made P)
int segment_locked(loamx_ctx* ctx, const void* d_scans, bool f32, size_t n_scans, const SegParams& P, const SegOutputs& out) {
  const size_t cells = n_scans * (size_t)P.H * P.W, nb = ((size_t)P.H * P.W + kSegBlock - 1) / kSegBlock;
  const size_t cells16 = round16(cells);
  ENSURE(ctx, WS_SEG_BYTES, 2 * cells16);
  ENSURE(ctx, WS_SEG_WORDS, (4 * cells16 + n_scans * nb) * sizeof(uint32_t));
  const size_t count_bytes = round16(n_scans * (kSegStatWords + 1) * sizeof(uint32_t));
  ENSURE(ctx, WS_SEG_COUNTS, count_bytes);
  untimed(ctx);
  SegScratch ws;
  ws.cls = wsp<uint8_t>(ctx, WS_SEG_BYTES), ws.ebits = ws.cls + cells16;
  ws.parent = wsp<uint32_t>(ctx, WS_SEG_WORDS), ws.root = ws.parent + cells16, ws.size = ws.root + cells16;
  ws.line_max = ws.size + cells16, ws.block_cnt = ws.line_max + cells16;
  ws.edges = wsp<uint32_t>(ctx, WS_SEG_COUNTS), ws.stats = ws.edges + n_scans;
  HIP_TRY(ctx, hipMemsetAsync(ctx->ws[WS_SEG_COUNTS].p, 0, count_bytes, ctx->stream));
  const bool tiles = !(ctx->reg_flags & kRegFlagNoSegmentTiles);
  launch_segment(d_scans, f32, (uint32_t)n_scans, P, tiles, ws, out, ctx->stream);
  CHECK_LAUNCH(ctx, "segment kernels");
  ctx->last_segment.valid = true, ctx->last_segment.tiles = tiles;
  ctx->last_segment.H = P.H, ctx->last_segment.W = P.W, ctx->last_segment.n_scans = (uint32_t)n_scans;
  return LOAMX_OK;
}

int segment_scans_dev(loamx_ctx* ctx, const void* d_scans, bool f32, size_t n_scans, const loamx_lidar_params* lidar,
                      const loamx_segment_params* params, uint8_t* d_classes, uint32_t* d_labels, uint32_t* d_sizes, void* d_filtered,
                      loamx_segment_cluster* d_clusters, size_t max_clusters, uint32_t* d_stats) {
  API_ENTER(ctx);
  SegParams P;
  int rc = make_segment_params(ctx, lidar, params, n_scans, P);
  if (rc != LOAMX_OK || n_scans == 0) return rc;
  if (!d_scans) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null scans");
  return segment_locked(ctx, d_scans, f32, n_scans, P, SegOutputs{d_classes, d_labels, d_sizes, d_filtered, d_clusters, max_clusters, d_stats});
}

// host memory in, host memory out: upload, the device path on one scan, download, synchronise
int segment_scan_host(loamx_ctx* ctx, const void* scan, bool f32, const loamx_lidar_params* lidar, const loamx_segment_params* params,
                      uint8_t* classes, uint32_t* labels, uint32_t* sizes, void* filtered, loamx_segment_cluster* clusters, size_t max_clusters,
                      uint32_t* stats) {
  API_ENTER(ctx);
  SegParams P;
  int rc = make_segment_params(ctx, lidar, params, 1, P);
  if (rc != LOAMX_OK) return rc;
  if (!scan) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null scan");
  const size_t HW = (size_t)P.H * P.W, scan_bytes = HW * 3 * (f32 ? sizeof(float) : sizeof(double));
  if (max_clusters > HW) max_clusters = HW;  // (a scan has at most HW components)
  const size_t rec_bytes = max_clusters * sizeof(loamx_segment_cluster);
  // the device copies: the filtered scan is made in place in the uploaded one
  const size_t o_labels = 0, o_sizes = o_labels + round16(HW * 4), o_clusters = o_sizes + round16(HW * 4), o_stats = o_clusters + round16(rec_bytes);
  const size_t o_classes = o_stats + round16(kSegStatWords * 4), out_bytes = o_classes + round16(HW);
  untimed(ctx);
  ENSURE(ctx, WS_SEG_IN, scan_bytes);
  ENSURE(ctx, WS_SEG_OUT, out_bytes);
  unsigned char* d_out = wsp<unsigned char>(ctx, WS_SEG_OUT);
  HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[WS_SEG_IN].p, scan, scan_bytes, hipMemcpyHostToDevice, ctx->stream));
  SegOutputs out{};
  out.classes = classes ? d_out + o_classes : nullptr;
  out.labels = labels ? reinterpret_cast<uint32_t*>(d_out + o_labels) : nullptr;
  out.sizes = sizes ? reinterpret_cast<uint32_t*>(d_out + o_sizes) : nullptr;
  out.filtered = filtered ? ctx->ws[WS_SEG_IN].p : nullptr;
  out.clusters = clusters ? reinterpret_cast<loamx_segment_cluster*>(d_out + o_clusters) : nullptr;
  out.max_clusters = max_clusters;
  out.stats = reinterpret_cast<uint32_t*>(d_out + o_stats);  // (always: the number of records to bring back)
  rc = segment_locked(ctx, ctx->ws[WS_SEG_IN].p, f32, 1, P, out);
  if (rc != LOAMX_OK) {
    (void)hipStreamSynchronize(ctx->stream);  // (the upload must not outlive the caller's array)
    return rc;
  }
  uint32_t st[kSegStatWords];
  HIP_TRY(ctx, hipMemcpyAsync(st, out.stats, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
  if (classes) HIP_TRY(ctx, hipMemcpyAsync(classes, out.classes, HW, hipMemcpyDeviceToHost, ctx->stream));
  if (labels) HIP_TRY(ctx, hipMemcpyAsync(labels, out.labels, HW * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (sizes) HIP_TRY(ctx, hipMemcpyAsync(sizes, out.sizes, HW * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (filtered) HIP_TRY(ctx, hipMemcpyAsync(filtered, out.filtered, scan_bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (clusters && st[7]) HIP_TRY(ctx, hipMemcpy(clusters, out.clusters, (size_t)st[7] * sizeof(loamx_segment_cluster), hipMemcpyDeviceToHost));
  if (stats) memcpy(stats, st, sizeof(st));
  return LOAMX_OK;
}

}  // namespace

extern "C" {

void loamx_default_segment_params(loamx_segment_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->ground_lines = 0, p->ground_angle = 10.0 * M_PI / 180.0, p->segment_angle = 60.0 * M_PI / 180.0;
  p->min_cluster_points = 30, p->min_tall_cluster_points = 5, p->min_tall_cluster_lines = 3;
  p->drop_outliers = 1, p->drop_ground = 0;
}

int loamx_segment_constants(const loamx_segment_params* params, double out[2]) {
  if (!out) return LOAMX_ERR_BAD_PARAM;
  const char* why = "";
  return segment_constants(params, out, &why);
}

int loamx_segment_scans_dev(loamx_ctx* ctx, const double* d_scans, size_t n_scans, const loamx_lidar_params* lidar,
                            const loamx_segment_params* params, uint8_t* d_classes, uint32_t* d_labels, uint32_t* d_sizes, double* d_filtered,
                            loamx_segment_cluster* d_clusters, size_t max_clusters, uint32_t* d_stats) {
  return segment_scans_dev(ctx, d_scans, false, n_scans, lidar, params, d_classes, d_labels, d_sizes, d_filtered, d_clusters, max_clusters, d_stats);
}
int loamx_segment_scans_dev_f32(loamx_ctx* ctx, const float* d_scans, size_t n_scans, const loamx_lidar_params* lidar,
                                const loamx_segment_params* params, uint8_t* d_classes, uint32_t* d_labels, uint32_t* d_sizes, float* d_filtered,
                                loamx_segment_cluster* d_clusters, size_t max_clusters, uint32_t* d_stats) {
  return segment_scans_dev(ctx, d_scans, true, n_scans, lidar, params, d_classes, d_labels, d_sizes, d_filtered, d_clusters, max_clusters, d_stats);
}
int loamx_segment_scan(loamx_ctx* ctx, const double* scan, const loamx_lidar_params* lidar, const loamx_segment_params* params, uint8_t* classes,
                       uint32_t* labels, uint32_t* sizes, double* filtered, loamx_segment_cluster* clusters, size_t max_clusters, uint32_t* stats) {
  return segment_scan_host(ctx, scan, false, lidar, params, classes, labels, sizes, filtered, clusters, max_clusters, stats);
}
int loamx_segment_scan_f32(loamx_ctx* ctx, const float* scan, const loamx_lidar_params* lidar, const loamx_segment_params* params, uint8_t* classes,
                           uint32_t* labels, uint32_t* sizes, float* filtered, loamx_segment_cluster* clusters, size_t max_clusters, uint32_t* stats) {
  return segment_scan_host(ctx, scan, true, lidar, params, classes, labels, sizes, filtered, clusters, max_clusters, stats);
}

int loamx_ctx_last_segment_census(loamx_ctx* ctx, uint64_t out[5]) {
  API_ENTER(ctx);
  if (!out) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  if (!ctx->last_segment.valid) return fail(ctx, LOAMX_ERR_BAD_PARAM, "no segmentation call on this context yet");
  const auto& ls = ctx->last_segment;
  std::vector<uint32_t> edges(ls.n_scans);
  HIP_TRY(ctx, hipMemcpyAsync(edges.data(), ctx->ws[WS_SEG_COUNTS].p, edges.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  out[0] = kSegTileLines, out[1] = kSegTileCols;
  out[2] = (uint64_t)((ls.H + kSegTileLines - 1) / kSegTileLines) * ((ls.W + kSegTileCols - 1) / kSegTileCols);
  out[3] = 0;
  for (uint32_t e : edges) out[3] += e;
  out[4] = ls.tiles ? 1 : 0;
  return LOAMX_OK;
}

}  // extern "C"
