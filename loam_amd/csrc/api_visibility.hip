// api_visibility.hip — map cleaning (loamx.h, "map cleaning"): the visibility votes of map points over posed scans in their
// device and host forms, the decision with its ordered compaction, and the census of the last votes call.
#include "api_host.h"
#include "visibility_math.h"

using namespace loamx;

namespace {

int params_check(loamx_ctx* ctx, const loamx_visibility_params* p) {
  if (!p) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null visibility params");
  if (!isfinite(p->min_range) || !isfinite(p->max_range) || !isfinite(p->margin) || !isfinite(p->margin_rel) || !isfinite(p->through_ratio))
    return fail(ctx, LOAMX_ERR_BAD_PARAM, "a visibility parameter is not finite");
  if (p->min_range < 0.0) return fail(ctx, LOAMX_ERR_BAD_PARAM, "min_range must not be negative");
  if (p->max_range < p->min_range) return fail(ctx, LOAMX_ERR_BAD_PARAM, "max_range must be at least min_range");
  if (p->margin < 0.0 || p->margin_rel < 0.0) return fail(ctx, LOAMX_ERR_BAD_PARAM, "margin and margin_rel must not be negative");
  if (p->through_ratio < 0.0) return fail(ctx, LOAMX_ERR_BAD_PARAM, "through_ratio must not be negative");
  if (p->window_lines > 3 || p->window_cols > 3) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "a visibility window of more than 3 cells each way");
  return LOAMX_OK;
}

VisRule make_rule(const loamx_visibility_params* p) {
  VisRule r;
  r.min2 = p->min_range * p->min_range, r.max2 = p->max_range * p->max_range;
  r.margin = p->margin, r.margin_rel = p->margin_rel;
  r.window_lines = p->window_lines, r.window_cols = p->window_cols;
  return r;
}

// the argument checks the device and the host forms share
int votes_check(loamx_ctx* ctx, const loamx_scan_layout* l, const void* points, size_t stride, size_t n_points, const void* scans, size_t n_scans,
                const void* poses, const loamx_visibility_params* params, const void* votes) {
  if (!l) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null scan layout");
  if (l->device != ctx->device) return fail(ctx, LOAMX_ERR_BAD_PARAM, "the scan layout was created on another device");
  int rc = params_check(ctx, params);
  if (rc != LOAMX_OK) return rc;
  if (stride < 3) return fail(ctx, LOAMX_ERR_BAD_PARAM, "point_stride must be >= 3");
  if (stride > 0xFFFFFFFFull) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "point_stride does not fit 32 bits");
  if (n_points > 0xFFFFFFFFull) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "2^32 map points or more");
  if (n_scans > 0x7FFFFFFFull) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "2^31 scans or more");
  if (n_scans && !poses) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null poses");
  if (n_scans && !scans) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null scans");
  if (n_points && (!points || !votes)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null points or votes");
  return LOAMX_OK;
}

// the caller holds ctx->mu, has selected the device and checked the arguments
int votes_locked(loamx_ctx* ctx, const loamx_scan_layout* l, const double* d_points, size_t stride, size_t n_points, const void* d_scans, bool f32,
                 size_t n_scans, const double* d_poses, const loamx_visibility_params* params, bool accumulate, loamx_visibility_tally* d_votes) {
  const bool ranges = !(ctx->reg_flags & kRegFlagNoVisibilityRanges);
  uint32_t chunk = kVisScanChunk;
  if ((n_scans + chunk - 1) / chunk > 65535u) chunk = (uint32_t)((n_scans + 65534u) / 65535u);
  const uint32_t n_chunks = n_scans ? (uint32_t)((n_scans + chunk - 1) / chunk) : 0u;
  ctx->last_visibility.valid = true, ctx->last_visibility.counted = false;
  ctx->last_visibility.form = ranges ? 1u : 0u, ctx->last_visibility.scan_chunks = n_chunks;
  if (n_points == 0) return LOAMX_OK;
  untimed(ctx);
  if (n_scans == 0) {
    if (!accumulate) HIP_TRY(ctx, hipMemsetAsync(d_votes, 0, n_points * sizeof(loamx_visibility_tally), ctx->stream));
    return LOAMX_OK;
  }
  const size_t n_cells = n_scans * (size_t)l->H * l->W;
  ENSURE(ctx, WS_VIS_CENSUS, 2 * sizeof(unsigned long long));
  if (ranges) ENSURE(ctx, WS_VIS_RANGES, n_cells * sizeof(double));
  HIP_TRY(ctx, hipMemsetAsync(ctx->ws[WS_VIS_CENSUS].p, 0, 2 * sizeof(unsigned long long), ctx->stream));
  VisVotesCall c;
  c.d_points = d_points, c.stride = (uint32_t)stride, c.n_points = (uint32_t)n_points;
  c.d_scans = d_scans, c.f32 = f32, c.d_ranges = ranges ? wsp<double>(ctx, WS_VIS_RANGES) : nullptr;
  c.n_scans = (uint32_t)n_scans, c.chunk = chunk, c.d_poses = d_poses;
  c.tab = OrgTables{l->d_col_dirs, l->d_line_tans, nullptr, 0u, l->H, l->W, l->clockwise};
  c.rule = make_rule(params);
  c.atomic = accumulate || n_chunks > 1;
  c.d_votes = d_votes, c.d_census = wsp<unsigned long long>(ctx, WS_VIS_CENSUS);
  if (c.atomic && !accumulate) HIP_TRY(ctx, hipMemsetAsync(d_votes, 0, n_points * sizeof(loamx_visibility_tally), ctx->stream));
  if (ranges) launch_visibility_ranges(d_scans, f32, n_cells, c.rule.min2, wsp<double>(ctx, WS_VIS_RANGES), ctx->stream);
  launch_visibility_votes(c, ctx->stream);
  CHECK_LAUNCH(ctx, "visibility kernels");
  ctx->last_visibility.counted = true;
  return LOAMX_OK;
}

int votes_dev(loamx_ctx* ctx, const loamx_scan_layout* l, const double* d_points, size_t stride, size_t n_points, const void* d_scans, bool f32,
              size_t n_scans, const double* d_poses, const loamx_visibility_params* params, int accumulate, loamx_visibility_tally* d_votes) {
  API_ENTER(ctx);
  int rc = votes_check(ctx, l, d_points, stride, n_points, d_scans, n_scans, d_poses, params, d_votes);
  if (rc != LOAMX_OK) return rc;
  return votes_locked(ctx, l, d_points, stride, n_points, d_scans, f32, n_scans, d_poses, params, accumulate != 0, d_votes);
}

// host memory in, host memory out: upload, the device path, download, synchronise
int votes_host(loamx_ctx* ctx, const loamx_scan_layout* l, const double* points, size_t stride, size_t n_points, const void* scans, bool f32,
               size_t n_scans, const double* poses, const loamx_visibility_params* params, loamx_visibility_tally* votes) {
  API_ENTER(ctx);
  int rc = votes_check(ctx, l, points, stride, n_points, scans, n_scans, poses, params, votes);
  if (rc != LOAMX_OK) return rc;
  const size_t pts_bytes = n_points * stride * sizeof(double), out_bytes = n_points * sizeof(loamx_visibility_tally);
  const size_t scan_bytes = n_scans * (size_t)l->H * l->W * 3 * (f32 ? sizeof(float) : sizeof(double)), pose_bytes = n_scans * 7 * sizeof(double);
  untimed(ctx);
  ENSURE(ctx, WS_VIS_IN, pts_bytes ? pts_bytes : 8);
  ENSURE(ctx, WS_VIS_SCANS, scan_bytes ? scan_bytes : 8);
  ENSURE(ctx, WS_VIS_POSES, pose_bytes ? pose_bytes : 8);
  ENSURE(ctx, WS_VIS_OUT, out_bytes ? out_bytes : 8);
  if (pts_bytes) HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[WS_VIS_IN].p, points, pts_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (scan_bytes) HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[WS_VIS_SCANS].p, scans, scan_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (pose_bytes) HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[WS_VIS_POSES].p, poses, pose_bytes, hipMemcpyHostToDevice, ctx->stream));
  rc = votes_locked(ctx, l, wsp<double>(ctx, WS_VIS_IN), stride, n_points, ctx->ws[WS_VIS_SCANS].p, f32, n_scans, wsp<double>(ctx, WS_VIS_POSES), params,
                    false, wsp<loamx_visibility_tally>(ctx, WS_VIS_OUT));
  if (rc != LOAMX_OK) {
    (void)hipStreamSynchronize(ctx->stream);  // (the uploads must not outlive the caller's arrays)
    return rc;
  }
  if (out_bytes) HIP_TRY(ctx, hipMemcpyAsync(votes, ctx->ws[WS_VIS_OUT].p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LOAMX_OK;
}

}  // namespace

extern "C" {

void loamx_default_visibility_params(loamx_visibility_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->min_range = 1.0, p->max_range = 80.0, p->margin = 0.3, p->margin_rel = 0.01;
  p->window_lines = 1, p->window_cols = 1, p->min_through = 2, p->through_ratio = 1.0;
}

int loamx_visibility_votes_dev(loamx_ctx* ctx, const loamx_scan_layout* layout, const double* d_points, size_t point_stride, size_t n_points,
                               const double* d_scans, size_t n_scans, const double* d_poses, const loamx_visibility_params* params, int accumulate,
                               loamx_visibility_tally* d_votes) {
  return votes_dev(ctx, layout, d_points, point_stride, n_points, d_scans, false, n_scans, d_poses, params, accumulate, d_votes);
}
int loamx_visibility_votes_dev_f32(loamx_ctx* ctx, const loamx_scan_layout* layout, const double* d_points, size_t point_stride, size_t n_points,
                                   const float* d_scans, size_t n_scans, const double* d_poses, const loamx_visibility_params* params, int accumulate,
                                   loamx_visibility_tally* d_votes) {
  return votes_dev(ctx, layout, d_points, point_stride, n_points, d_scans, true, n_scans, d_poses, params, accumulate, d_votes);
}
int loamx_visibility_votes(loamx_ctx* ctx, const loamx_scan_layout* layout, const double* points, size_t point_stride, size_t n_points,
                           const double* scans, size_t n_scans, const double* poses, const loamx_visibility_params* params,
                           loamx_visibility_tally* votes) {
  return votes_host(ctx, layout, points, point_stride, n_points, scans, false, n_scans, poses, params, votes);
}
int loamx_visibility_votes_f32(loamx_ctx* ctx, const loamx_scan_layout* layout, const double* points, size_t point_stride, size_t n_points,
                               const float* scans, size_t n_scans, const double* poses, const loamx_visibility_params* params,
                               loamx_visibility_tally* votes) {
  return votes_host(ctx, layout, points, point_stride, n_points, scans, true, n_scans, poses, params, votes);
}

int loamx_visibility_filter_dev(loamx_ctx* ctx, const loamx_visibility_tally* d_votes, size_t n_points, const loamx_visibility_params* params,
                                const double* d_points, size_t point_stride, uint8_t* d_dynamic_out, double* d_static_xyz_out,
                                uint32_t* d_static_index_out, size_t capacity, uint32_t* d_n_static_out) {
  API_ENTER(ctx);
  int rc = params_check(ctx, params);
  if (rc != LOAMX_OK) return rc;
  if (!d_n_static_out) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null d_n_static_out");
  if (n_points > 0xFFFFFFFFull) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "2^32 map points or more");
  if (n_points && !d_votes) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null votes");
  if (d_points && point_stride < 3) return fail(ctx, LOAMX_ERR_BAD_PARAM, "point_stride must be >= 3");
  if (d_points && point_stride > 0xFFFFFFFFull) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "point_stride does not fit 32 bits");
  if (d_points && capacity && !d_static_xyz_out) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null d_static_xyz_out with points and a capacity");
  untimed(ctx);
  ENSURE(ctx, WS_VIS_KEEP, n_points ? n_points : 8);
  ENSURE(ctx, WS_VIS_TILES, map_compact_ws_bytes(n_points ? n_points : 1));
  launch_visibility_filter(d_votes, (uint32_t)n_points, params->min_through, params->through_ratio, d_points, (uint32_t)point_stride,
                           wsp<uint8_t>(ctx, WS_VIS_KEEP), wsp<uint32_t>(ctx, WS_VIS_TILES), d_dynamic_out, d_points ? d_static_xyz_out : nullptr,
                           d_static_index_out, capacity, d_n_static_out, ctx->stream);
  CHECK_LAUNCH(ctx, "visibility filter kernels");
  return LOAMX_OK;
}

int loamx_ctx_last_visibility_census(loamx_ctx* ctx, loamx_visibility_census* out) {
  API_ENTER(ctx);
  if (!out) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  if (!ctx->last_visibility.valid) return fail(ctx, LOAMX_ERR_BAD_PARAM, "no visibility votes call on this context yet");
  unsigned long long words[2] = {0, 0};
  if (ctx->last_visibility.counted) {
    untimed(ctx);
    HIP_TRY(ctx, hipMemcpyAsync(words, ctx->ws[WS_VIS_CENSUS].p, sizeof(words), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  out->form = ctx->last_visibility.form, out->scan_chunks = ctx->last_visibility.scan_chunks;
  out->in_range_pairs = words[0], out->projected_pairs = words[1];
  return LOAMX_OK;
}

}  // extern "C"
