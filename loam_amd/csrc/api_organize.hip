// api_organize.hip — unordered clouds into organised scans (loamx.h, "unordered clouds into scans"): the scan layout with its
// two host-computed tables, the device-resident batch entry points and the one-cloud host forms.
#include "api_host.h"

using namespace loamx;

namespace {

void layout_free(loamx_scan_layout* l) {
  if (l->d_col_dirs) (void)hipFree(l->d_col_dirs);
  if (l->d_line_tans) (void)hipFree(l->d_line_tans);
  if (l->d_ring_map) (void)hipFree(l->d_ring_map);
  delete l;
}

OrgTables layout_tables(const loamx_scan_layout* l) {
  return OrgTables{l->d_col_dirs, l->d_line_tans, l->d_ring_map, (uint32_t)l->ring_map.size(), l->H, l->W, l->clockwise};
}

// the clouds of the call chunk by chunk (the caller holds ctx->mu, has selected the device and checked the arguments)
int organize_locked(loamx_ctx* ctx, const loamx_scan_layout* l, const void* d_points, bool f32, size_t stride, const uint16_t* d_rings,
                    const size_t* offsets, size_t n_clouds, void* d_scans, uint32_t* d_src_idx, uint32_t* d_stats) {
  const size_t HW = (size_t)l->H * l->W, scalar = f32 ? sizeof(float) : sizeof(double);
  const bool nearest = l->keep == LOAMX_ORGANIZE_KEEP_NEAREST;
  // the workspace of the largest chunk, before anything is enqueued
  size_t most_clouds = 0, most_points = 0;
  for (CloudChunks ch(offsets, n_clouds); ch.next();) {
    most_clouds = ch.nc > most_clouds ? ch.nc : most_clouds;
    most_points = ch.offs.off[ch.nc] - ch.offs.off[0] > most_points ? ch.offs.off[ch.nc] - ch.offs.off[0] : most_points;
  }
  ENSURE(ctx, WS_ORG_WINNER, most_clouds * HW * sizeof(uint32_t));
  ENSURE(ctx, WS_ORG_COUNTS, most_clouds * kOrgCounterWords * sizeof(uint32_t));
  if (nearest) {
    ENSURE(ctx, WS_ORG_RANGE, most_clouds * HW * sizeof(unsigned long long));
    ENSURE(ctx, WS_ORG_CELL, (most_points ? most_points : 1) * sizeof(uint32_t));
  }
  untimed(ctx);
  const OrgTables L = layout_tables(l);
  for (CloudChunks ch(offsets, n_clouds); ch.next();) {
    HIP_TRY(ctx, hipMemsetAsync(ctx->ws[WS_ORG_WINNER].p, 0xFF, ch.nc * HW * sizeof(uint32_t), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->ws[WS_ORG_COUNTS].p, 0, ch.nc * kOrgCounterWords * sizeof(uint32_t), ctx->stream));
    if (nearest) HIP_TRY(ctx, hipMemsetAsync(ctx->ws[WS_ORG_RANGE].p, 0xFF, ch.nc * HW * sizeof(unsigned long long), ctx->stream));
    launch_organize(d_points, f32, (uint32_t)stride, d_rings, ch.offs, ch.nc, ch.largest, L, nearest, wsp<uint32_t>(ctx, WS_ORG_WINNER),
                    wsp<unsigned long long>(ctx, WS_ORG_RANGE), wsp<uint32_t>(ctx, WS_ORG_CELL), wsp<uint32_t>(ctx, WS_ORG_COUNTS),
                    static_cast<unsigned char*>(d_scans) + ch.c0 * HW * 3 * scalar, d_src_idx ? d_src_idx + ch.c0 * HW : nullptr,
                    d_stats ? d_stats + ch.c0 * 4 : nullptr, ctx->stream);
    CHECK_LAUNCH(ctx, "organize kernels");
  }
  return LOAMX_OK;
}

// the argument checks the device and the host forms share; *empty: nothing to do
int organize_check(loamx_ctx* ctx, const loamx_scan_layout* l, const void* points, size_t stride, const size_t* offsets, size_t n_clouds,
                   const void* scans, bool* empty) {
  *empty = n_clouds == 0;
  if (!l) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null scan layout");
  if (l->device != ctx->device) return fail(ctx, LOAMX_ERR_BAD_PARAM, "the scan layout was created on another device");
  if (stride < 3) return fail(ctx, LOAMX_ERR_BAD_PARAM, "point_stride must be >= 3");
  if (stride > 0xFFFFFFFFull) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "point_stride does not fit 32 bits");
  if (n_clouds == 0) return LOAMX_OK;
  if (!offsets || !scans) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  for (size_t c = 0; c < n_clouds; c++) {
    if (offsets[c + 1] < offsets[c]) return fail(ctx, LOAMX_ERR_BAD_PARAM, "cloud_offsets must ascend");
    if (offsets[c + 1] - offsets[c] > 0xFFFFFFFEull) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "a cloud of more than 2^32 - 2 points");
  }
  if (offsets[n_clouds] > offsets[0] && !points) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null points");
  return LOAMX_OK;
}

int organize_clouds_dev(loamx_ctx* ctx, const loamx_scan_layout* l, const void* d_points, bool f32, size_t stride, const uint16_t* d_rings,
                        const size_t* offsets, size_t n_clouds, void* d_scans, uint32_t* d_src_idx, uint32_t* d_stats) {
  API_ENTER(ctx);
  bool empty;
  int rc = organize_check(ctx, l, d_points, stride, offsets, n_clouds, d_scans, &empty);
  if (rc != LOAMX_OK || empty) return rc;
  if (!d_points) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null points");
  return organize_locked(ctx, l, d_points, f32, stride, d_rings, offsets, n_clouds, d_scans, d_src_idx, d_stats);
}

// host memory in, host memory out: upload, the device path on one cloud, download, synchronise
int organize_cloud_host(loamx_ctx* ctx, const loamx_scan_layout* l, const void* points, bool f32, size_t stride, const uint16_t* rings, size_t n,
                        void* scan, uint32_t* src_idx, uint32_t* stats) {
  API_ENTER(ctx);
  const size_t offsets[2] = {0, n};
  bool empty;
  int rc = organize_check(ctx, l, points, stride, offsets, 1, scan, &empty);
  if (rc != LOAMX_OK) return rc;
  const size_t HW = (size_t)l->H * l->W, scalar = f32 ? sizeof(float) : sizeof(double);
  const size_t in_bytes = n * stride * scalar, scan_bytes = HW * 3 * scalar, idx_bytes = HW * sizeof(uint32_t);
  untimed(ctx);
  ENSURE(ctx, WS_ORG_IN, in_bytes ? in_bytes : 8);
  if (rings) ENSURE(ctx, WS_ORG_RINGS, n ? n * sizeof(uint16_t) : 8);
  ENSURE(ctx, WS_ORG_OUT, scan_bytes + idx_bytes + 4 * sizeof(uint32_t));
  unsigned char* d_out = wsp<unsigned char>(ctx, WS_ORG_OUT);
  uint32_t* d_idx = reinterpret_cast<uint32_t*>(d_out + scan_bytes);
  uint32_t* d_st = d_idx + HW;
  if (n) HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[WS_ORG_IN].p, points, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (n && rings) HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[WS_ORG_RINGS].p, rings, n * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream));
  rc = organize_locked(ctx, l, ctx->ws[WS_ORG_IN].p, f32, stride, rings ? wsp<uint16_t>(ctx, WS_ORG_RINGS) : nullptr, offsets, 1, d_out, d_idx, d_st);
  if (rc != LOAMX_OK) {
    (void)hipStreamSynchronize(ctx->stream);  // (the uploads must not outlive the caller's arrays)
    return rc;
  }
  HIP_TRY(ctx, hipMemcpyAsync(scan, d_out, scan_bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (src_idx) HIP_TRY(ctx, hipMemcpyAsync(src_idx, d_idx, idx_bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (stats) HIP_TRY(ctx, hipMemcpyAsync(stats, d_st, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LOAMX_OK;
}

}  // namespace

extern "C" {

void loamx_default_organize_params(loamx_organize_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->azimuth_zero = 0.0, p->clockwise = 0, p->keep = LOAMX_ORGANIZE_KEEP_FIRST;
  p->elevations = nullptr, p->fov_bottom = -15.0 * M_PI / 180.0, p->fov_top = 15.0 * M_PI / 180.0;
  p->ring_map = nullptr, p->n_ring_map = 0;
}

int loamx_scan_layout_create(loamx_ctx* ctx, const loamx_lidar_params* lidar, const loamx_organize_params* params, loamx_scan_layout** out) {
  API_ENTER(ctx);
  if (!lidar || !params || !out) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  *out = nullptr;
  if (lidar->scan_lines == 0 || lidar->points_per_line == 0) return fail(ctx, LOAMX_ERR_BAD_PARAM, "scan_lines and points_per_line must be >= 1");
  // (the limits make_extract_params applies to a lidar shape: whatever is organised here can be extracted)
  if (lidar->points_per_line > (uint64_t)kMaxLineWidth) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "points_per_line > 4096 not supported by the kernels");
  if (lidar->scan_lines > 0xFFFFFFFFull || lidar->scan_lines * lidar->points_per_line > 0xFFFFFFFFull / 4)
    return fail(ctx, LOAMX_ERR_UNSUPPORTED, "scan too large for 32-bit point indices");
  if (params->keep != LOAMX_ORGANIZE_KEEP_FIRST && params->keep != LOAMX_ORGANIZE_KEEP_NEAREST) return fail(ctx, LOAMX_ERR_BAD_PARAM, "unknown keep rule");
  if (!isfinite(params->azimuth_zero)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "azimuth_zero is not finite");
  if (params->n_ring_map && !params->ring_map) return fail(ctx, LOAMX_ERR_BAD_PARAM, "n_ring_map without a ring_map");
  const uint32_t H = (uint32_t)lidar->scan_lines, W = (uint32_t)lidar->points_per_line;
  loamx_scan_layout* l = new loamx_scan_layout;
  l->device = ctx->device, l->H = H, l->W = W, l->clockwise = params->clockwise ? 1u : 0u, l->keep = params->keep;
  auto refuse = [&](const char* msg) {
    layout_free(l);
    return fail(ctx, LOAMX_ERR_BAD_PARAM, msg);
  };
  l->col_dirs.resize(2 * (size_t)W);
  organize_column_dirs(params->azimuth_zero, l->clockwise != 0, W, l->col_dirs.data());
  std::vector<double> el(H, 0.0);
  if (params->elevations) {
    for (uint32_t i = 0; i < H; i++) el[i] = params->elevations[i];
  } else if (H > 1) {
    if (!isfinite(params->fov_bottom) || !isfinite(params->fov_top)) return refuse("fov_bottom / fov_top is not finite");
    if (!(params->fov_top > params->fov_bottom)) return refuse("fov_top must lie above fov_bottom");
    for (uint32_t i = 0; i < H; i++) el[i] = organize_linear_elevation(params->fov_bottom, params->fov_top, H, i);
  }
  l->line_tans.resize((size_t)H + 1);
  if (const char* why = organize_line_tans(el.data(), H, l->line_tans.data())) return refuse(why);
  if (params->n_ring_map) {
    l->ring_map.assign(params->ring_map, params->ring_map + params->n_ring_map);
    for (uint16_t v : l->ring_map)
      if (v != 0xFFFFu && v >= H) return refuse("a ring_map entry names a line >= scan_lines");
  }
  auto upload = [&](auto** d, const auto& v) -> hipError_t {
    hipError_t e = hipMalloc(reinterpret_cast<void**>(d), v.size() * sizeof(v[0]));
    if (e == hipSuccess) e = hipMemcpy(*d, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice);
    return e;
  };
  hipError_t e = upload(&l->d_col_dirs, l->col_dirs);
  if (e == hipSuccess) e = upload(&l->d_line_tans, l->line_tans);
  if (e == hipSuccess && !l->ring_map.empty()) e = upload(&l->d_ring_map, l->ring_map);
  if (e != hipSuccess) {
    layout_free(l);
    return fail(ctx, LOAMX_ERR_HIP, std::string("scan layout tables: ") + hipGetErrorString(e));
  }
  *out = l;
  return LOAMX_OK;
}

void loamx_scan_layout_destroy(loamx_ctx* ctx, loamx_scan_layout* layout) {
  if (!layout) return;
  if (ctx) {
    std::lock_guard<std::mutex> guard(ctx->mu);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);  // (kernels still reading the tables)
    layout_free(layout);
    return;
  }
  layout_free(layout);
}

int loamx_scan_layout_tables(const loamx_scan_layout* layout, double* col_dirs, double* line_tans) {
  if (!layout) return LOAMX_ERR_BAD_PARAM;
  if (col_dirs) memcpy(col_dirs, layout->col_dirs.data(), layout->col_dirs.size() * sizeof(double));
  if (line_tans) memcpy(line_tans, layout->line_tans.data(), layout->line_tans.size() * sizeof(double));
  return LOAMX_OK;
}

int loamx_organize_clouds_dev(loamx_ctx* ctx, const loamx_scan_layout* layout, const double* d_points, size_t point_stride, const uint16_t* d_rings,
                              const size_t* cloud_offsets, size_t n_clouds, double* d_scans, uint32_t* d_src_idx, uint32_t* d_stats) {
  return organize_clouds_dev(ctx, layout, d_points, false, point_stride, d_rings, cloud_offsets, n_clouds, d_scans, d_src_idx, d_stats);
}
int loamx_organize_clouds_dev_f32(loamx_ctx* ctx, const loamx_scan_layout* layout, const float* d_points, size_t point_stride, const uint16_t* d_rings,
                                  const size_t* cloud_offsets, size_t n_clouds, float* d_scans, uint32_t* d_src_idx, uint32_t* d_stats) {
  return organize_clouds_dev(ctx, layout, d_points, true, point_stride, d_rings, cloud_offsets, n_clouds, d_scans, d_src_idx, d_stats);
}
int loamx_organize_cloud(loamx_ctx* ctx, const loamx_scan_layout* layout, const double* points, size_t point_stride, const uint16_t* rings,
                         size_t n_points, double* scan, uint32_t* src_idx, uint32_t* stats) {
  return organize_cloud_host(ctx, layout, points, false, point_stride, rings, n_points, scan, src_idx, stats);
}
int loamx_organize_cloud_f32(loamx_ctx* ctx, const loamx_scan_layout* layout, const float* points, size_t point_stride, const uint16_t* rings,
                             size_t n_points, float* scan, uint32_t* src_idx, uint32_t* stats) {
  return organize_cloud_host(ctx, layout, points, true, point_stride, rings, n_points, scan, src_idx, stats);
}

}  // extern "C"
