// api_raycast.hip — the occupancy ray cast (loamx.h, "occupancy ray casting"): the checks, the two device entry points, their host
// forms and the census of the context's last call. The kernels: raycast_kernels.hip; the map's handle: api_occupancy.h.
#include "api_occupancy.h"

using namespace loamx;

namespace {

constexpr unsigned long long kRayMaxRays = 1ull << 31;

int params_check(loamx_ctx* ctx, const loamx_occupancy_map* map, const loamx_raycast_params* params, RayRule* rule) {
  int rc = occupancy_map_check(ctx, map);
  if (rc != LOAMX_OK) return rc;
  if (!params) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null params");
  if (params->hit_at != LOAMX_RAY_AT_ENTER && params->hit_at != LOAMX_RAY_AT_MIDDLE) return fail(ctx, LOAMX_ERR_BAD_PARAM, "unknown hit_at");
  if (params->max_steps > kRayMaxSteps) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "max_steps > 2^22 not supported");
  rule->skip_start = params->skip_start, rule->unknown_stops = params->unknown_stops ? 1u : 0u;
  rule->max_steps = params->max_steps, rule->hit_at = params->hit_at;
  return LOAMX_OK;
}

int cast_check(loamx_ctx* ctx, const loamx_occupancy_map* map, const double* origins, const double* ends, size_t stride, size_t n,
               const loamx_raycast_params* params, const loamx_ray_record* records, RayRule* rule) {
  int rc = params_check(ctx, map, params, rule);
  if (rc != LOAMX_OK) return rc;
  if (stride < 3) return fail(ctx, LOAMX_ERR_BAD_PARAM, "stride must be >= 3");
  if (stride > 0xFFFFFFFFull) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "stride does not fit 32 bits");
  if (n && (!origins || !ends || !records)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null origins, ends or records");
  if (n > kRayMaxRays) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "a call casts at most 2^31 rays");
  return LOAMX_OK;
}

// *n: the rays of the call
int render_check(loamx_ctx* ctx, const loamx_occupancy_map* map, const double* dirs, size_t n_beams, const double* poses, size_t n_poses,
                 double max_range, const loamx_raycast_params* params, RayRule* rule, unsigned long long* n) {
  int rc = params_check(ctx, map, params, rule);
  if (rc != LOAMX_OK) return rc;
  if (!isfinite(max_range) || !(max_range > 0.0)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "max_range must be finite and positive");
  *n = 0;
  if (n_beams == 0 || n_poses == 0) return LOAMX_OK;
  if (n_beams > kRayMaxRays || n_poses > kRayMaxRays || (unsigned long long)n_beams * n_poses > kRayMaxRays)
    return fail(ctx, LOAMX_ERR_UNSUPPORTED, "a call renders at most 2^31 beams");
  if (!dirs || !poses) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null dirs or poses");
  *n = (unsigned long long)n_beams * n_poses;
  return LOAMX_OK;
}

void no_rays(loamx_ctx* ctx) { ctx->last_raycast.counted = false, ctx->last_raycast.rays = 0; }

// the census words of a call that is about to launch, zeroed on the stream
int census_begin(loamx_ctx* ctx, unsigned long long n) {
  untimed(ctx);
  ENSURE(ctx, WS_RAY_CENSUS, kRayCensusWords * sizeof(unsigned long long));
  HIP_TRY(ctx, hipMemsetAsync(ctx->ws[WS_RAY_CENSUS].p, 0, kRayCensusWords * sizeof(unsigned long long), ctx->stream));
  ctx->last_raycast.counted = true, ctx->last_raycast.rays = n;
  return LOAMX_OK;
}

int launch_cast(loamx_ctx* ctx, const loamx_occupancy_map* map, const RayRule& rule, const double* d_origins, const double* d_ends, size_t stride,
                size_t n, loamx_ray_record* d_records) {
  int rc = census_begin(ctx, n);
  if (rc != LOAMX_OK) return rc;
  launch_raycast(map->t, map->rule.leaf, map->state_rule, rule, d_origins, d_ends, (uint32_t)stride, n, reinterpret_cast<RayRecord*>(d_records),
                 wsp<unsigned long long>(ctx, WS_RAY_CENSUS), (ctx->reg_flags & kRegFlagRaycastCombine) != 0, ctx->stream);
  return check_launch(ctx, "ray cast kernel");
}

int launch_render(loamx_ctx* ctx, const loamx_occupancy_map* map, const RayRule& rule, const double* d_dirs, size_t n_beams, const double* d_poses,
                  size_t n_poses, double max_range, double* d_scans, double* d_ranges, loamx_ray_record* d_records) {
  int rc = census_begin(ctx, (unsigned long long)n_beams * n_poses);
  if (rc != LOAMX_OK) return rc;
  launch_raycast_render(map->t, map->rule.leaf, map->state_rule, rule, d_dirs, (uint32_t)n_beams, d_poses, n_poses, max_range, d_scans, d_ranges,
                        reinterpret_cast<RayRecord*>(d_records), wsp<unsigned long long>(ctx, WS_RAY_CENSUS),
                        (ctx->reg_flags & kRegFlagRaycastCombine) != 0, ctx->stream);
  return check_launch(ctx, "scan render kernel");
}

}  // namespace

extern "C" {

void loamx_default_raycast_params(loamx_raycast_params* p) {
  if (!p) return;
  p->skip_start = 0, p->unknown_stops = 0, p->max_steps = kRayDefaultMaxSteps, p->hit_at = LOAMX_RAY_AT_MIDDLE;
}

int loamx_occupancy_cast_rays(loamx_ctx* ctx, const loamx_occupancy_map* map, const double* d_origins, const double* d_ends, size_t stride, size_t n,
                              const loamx_raycast_params* params, loamx_ray_record* d_records_out) {
  API_ENTER(ctx);
  RayRule rule;
  int rc = cast_check(ctx, map, d_origins, d_ends, stride, n, params, d_records_out, &rule);
  if (rc != LOAMX_OK) return rc;
  if (n == 0) {
    no_rays(ctx);
    return LOAMX_OK;
  }
  return launch_cast(ctx, map, rule, d_origins, d_ends, stride, n, d_records_out);
}

int loamx_occupancy_render_scans(loamx_ctx* ctx, const loamx_occupancy_map* map, const double* d_dirs, size_t n_beams, const double* d_poses,
                                 size_t n_poses, double max_range, const loamx_raycast_params* params, double* d_scans_out, double* d_ranges_out,
                                 loamx_ray_record* d_records_out) {
  API_ENTER(ctx);
  RayRule rule;
  unsigned long long n = 0;
  int rc = render_check(ctx, map, d_dirs, n_beams, d_poses, n_poses, max_range, params, &rule, &n);
  if (rc != LOAMX_OK) return rc;
  if (n == 0) {
    no_rays(ctx);
    return LOAMX_OK;
  }
  return launch_render(ctx, map, rule, d_dirs, n_beams, d_poses, n_poses, max_range, d_scans_out, d_ranges_out, d_records_out);
}

int loamx_occupancy_cast_rays_host(loamx_ctx* ctx, const loamx_occupancy_map* map, const double* origins, const double* ends, size_t stride, size_t n,
                                   const loamx_raycast_params* params, loamx_ray_record* records_out) {
  API_ENTER(ctx);
  RayRule rule;
  int rc = cast_check(ctx, map, origins, ends, stride, n, params, records_out, &rule);
  if (rc != LOAMX_OK) return rc;
  if (n == 0) {
    no_rays(ctx);
    return LOAMX_OK;
  }
  if (n > (~(size_t)0) / (2 * stride * sizeof(double))) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "the segments do not fit the address space");
  const size_t in_bytes = n * stride * sizeof(double), o_ends = align256(in_bytes);
  untimed(ctx);
  ENSURE(ctx, WS_OCC_IN, o_ends + in_bytes);
  ENSURE(ctx, WS_OCC_OUT, n * sizeof(loamx_ray_record));
  char* in = static_cast<char*>(ctx->ws[WS_OCC_IN].p);
  HIP_TRY(ctx, hipMemcpyAsync(in, origins, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(in + o_ends, ends, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  rc = launch_cast(ctx, map, rule, reinterpret_cast<const double*>(in), reinterpret_cast<const double*>(in + o_ends), stride, n,
                   wsp<loamx_ray_record>(ctx, WS_OCC_OUT));
  if (rc != LOAMX_OK) {
    (void)hipStreamSynchronize(ctx->stream);  // (the uploads must not outlive the caller's arrays)
    return rc;
  }
  HIP_TRY(ctx, hipMemcpyAsync(records_out, ctx->ws[WS_OCC_OUT].p, n * sizeof(loamx_ray_record), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LOAMX_OK;
}

int loamx_occupancy_render_scans_host(loamx_ctx* ctx, const loamx_occupancy_map* map, const double* dirs, size_t n_beams, const double* poses,
                                      size_t n_poses, double max_range, const loamx_raycast_params* params, double* scans_out, double* ranges_out,
                                      loamx_ray_record* records_out) {
  API_ENTER(ctx);
  RayRule rule;
  unsigned long long n = 0;
  int rc = render_check(ctx, map, dirs, n_beams, poses, n_poses, max_range, params, &rule, &n);
  if (rc != LOAMX_OK) return rc;
  if (n == 0) {
    no_rays(ctx);
    return LOAMX_OK;
  }
  const size_t dir_bytes = n_beams * 3 * sizeof(double), pose_bytes = n_poses * 7 * sizeof(double);
  const size_t o_ranges = align256(n * 3 * sizeof(double)), o_records = o_ranges + align256(n * sizeof(double));
  untimed(ctx);
  ENSURE(ctx, WS_OCC_IN, dir_bytes);
  ENSURE(ctx, WS_OCC_POSE, pose_bytes);
  ENSURE(ctx, WS_OCC_OUT, o_records + n * sizeof(loamx_ray_record));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[WS_OCC_IN].p, dirs, dir_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[WS_OCC_POSE].p, poses, pose_bytes, hipMemcpyHostToDevice, ctx->stream));
  char* b = static_cast<char*>(ctx->ws[WS_OCC_OUT].p);
  rc = launch_render(ctx, map, rule, wsp<double>(ctx, WS_OCC_IN), n_beams, wsp<double>(ctx, WS_OCC_POSE), n_poses, max_range,
                     scans_out ? reinterpret_cast<double*>(b) : nullptr, ranges_out ? reinterpret_cast<double*>(b + o_ranges) : nullptr,
                     records_out ? reinterpret_cast<loamx_ray_record*>(b + o_records) : nullptr);
  if (rc != LOAMX_OK) {
    (void)hipStreamSynchronize(ctx->stream);  // (the uploads must not outlive the caller's arrays)
    return rc;
  }
  if (scans_out) HIP_TRY(ctx, hipMemcpyAsync(scans_out, b, n * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (ranges_out) HIP_TRY(ctx, hipMemcpyAsync(ranges_out, b + o_ranges, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (records_out) HIP_TRY(ctx, hipMemcpyAsync(records_out, b + o_records, n * sizeof(loamx_ray_record), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LOAMX_OK;
}

int loamx_ctx_last_raycast_census(loamx_ctx* ctx, loamx_raycast_census* out) {
  API_ENTER(ctx);
  if (!out) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  unsigned long long words[kRayCensusWords] = {};
  if (ctx->last_raycast.counted) {
    untimed(ctx);
    HIP_TRY(ctx, hipMemcpyAsync(words, ctx->ws[WS_RAY_CENSUS].p, sizeof(words), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  out->rays = ctx->last_raycast.rays, out->visits = words[kRayWordVisits], out->probes = words[kRayWordProbes];
  out->hit = words[kRayWordStatus + kRayHit], out->unknown = words[kRayWordStatus + kRayUnknown], out->clear = words[kRayWordStatus + kRayClear];
  out->truncated = words[kRayWordStatus + kRayTruncated], out->outside = words[kRayWordStatus + kRayOutside];
  out->invalid = words[kRayWordStatus + kRayInvalid];
  return LOAMX_OK;
}

}  // extern "C"
