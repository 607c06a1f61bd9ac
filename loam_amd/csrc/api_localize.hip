// api_localize.hip — surfel localisation (loamx.h, "surfel localisation"): the localiser handle with its one device block (plane
// cache, partial sums, per-cloud state), the run entry points and their host forms. Every launch of a call is enqueued up front;
// nothing is read back. On this handle the plain names are the device forms.
#include "api_listedmap.h"
#include "localize_math.h"

struct loamx_surfel_localizer {
  loamx_ctx* owner = nullptr;
  int device = 0;
  const loamx_surfel_map* map = nullptr;
  size_t max_clouds = 0, max_points = 0;
  void* block = nullptr;  // the one device allocation
  loamx::LocPlane* cache = nullptr;     // [2^log2_cap of the map's table]
  loamx::LocPartial* partials = nullptr;  // [localize_partials(max_points)]
  loamx::LocState* state = nullptr;     // [max_clouds]
};

using namespace loamx;

namespace {

static_assert(sizeof(loamx_localize_params) == 64, "loamx.h documents the size");
static_assert(sizeof(loamx_localize_result) == 128 && sizeof(LocResult) == 128, "loamx_localize_result is 128 bytes");
static_assert(offsetof(loamx_localize_result, iterations) == offsetof(LocResult, iterations) &&
                  offsetof(loamx_localize_result, used_mask) == offsetof(LocResult, used_mask) &&
                  offsetof(loamx_localize_result, final_cost) == offsetof(LocResult, final_cost),
              "LocResult is the layout of loamx_localize_result");
static_assert(LOAMX_LOCALIZE_CONVERGED == kLocConverged && LOAMX_LOCALIZE_MAX_ITERATIONS == kLocMaxIter &&
                  LOAMX_LOCALIZE_TOO_FEW_ROWS == kLocTooFewRows && LOAMX_LOCALIZE_NOT_FINITE == kLocNotFinite,
              "localize_math.h has the header's codes");
constexpr size_t kLocMaxClouds = (size_t)1 << 24;

bool good(double v) { return isfinite(v) && v >= 0.0; }

int run_check(loamx_ctx* ctx, const loamx_surfel_localizer* loc, const void* points, size_t stride, const size_t* offsets, size_t n_clouds,
              const void* poses_in, const void* poses_out, const void* results, const loamx_localize_params* p, size_t* total) {
  *total = 0;
  if (!loc) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null localiser");
  if (loc->owner != ctx) return fail(ctx, LOAMX_ERR_BAD_PARAM, "the localiser was created on another context");
  if (!p) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null params");
  if (stride < 3) return fail(ctx, LOAMX_ERR_BAD_PARAM, "point_stride must be >= 3");
  if (stride > 0xFFFFFFFFull) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "point_stride does not fit 32 bits");
  if (p->neighborhood != 1u && p->neighborhood != 7u) return fail(ctx, LOAMX_ERR_BAD_PARAM, "neighborhood must be 1 or 7");
  if (!good(p->planarity) || !good(p->max_distance) || !good(p->huber_delta) || !good(p->rotation_convergence_thresh) ||
      !good(p->position_convergence_thresh) || !good(p->min_eigenvalue_per_row))
    return fail(ctx, LOAMX_ERR_BAD_PARAM, "a localisation parameter is not finite or negative");
  if (p->max_iterations > kLocMaxIterations) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "max_iterations > 1000 not supported");
  if (n_clouds > loc->max_clouds) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "more clouds than the localiser was created for");
  if (n_clouds == 0) return LOAMX_OK;
  if (!offsets) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null cloud_offsets");
  for (size_t c = 0; c < n_clouds; c++)
    if (offsets[c + 1] < offsets[c]) return fail(ctx, LOAMX_ERR_BAD_PARAM, "cloud_offsets must ascend");
  *total = offsets[n_clouds] - offsets[0];
  if (*total > loc->max_points) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "more points than the localiser was created for");
  if (*total && !points) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null points");
  if (!poses_in || !poses_out || !results) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  return LOAMX_OK;
}

// the launches of a checked call; the caller holds ctx->mu and has selected the device
int run_locked(loamx_ctx* ctx, loamx_surfel_localizer* loc, const void* d_points, bool f32, size_t stride, const size_t* offsets, size_t n_clouds,
               const double* d_poses_in, double* d_poses_out, loamx_localize_result* d_results, loamx_reg_information* d_info,
               const loamx_localize_params* p) {
  const loamx_surfel_map* map = loc->map;
  LocRule R;
  R.leaf = map->rule.leaf, R.min_r2 = map->rule.min_r2, R.max_r2 = map->rule.max_r2;
  R.planarity = p->planarity, R.max_distance = p->max_distance == 0.0 ? map->rule.leaf : p->max_distance, R.huber_delta = p->huber_delta;
  R.min_points = p->min_points, R.neighborhood = p->neighborhood;
  LocSolve S;
  S.rot_thresh = p->rotation_convergence_thresh, S.pos_thresh = p->position_convergence_thresh, S.min_eig_per_row = p->min_eigenvalue_per_row;
  S.max_iterations = p->max_iterations, S.min_rows = p->min_rows;
  LocPlane* cache = (ctx->reg_flags & kRegFlagNoLocalizePlanes) ? nullptr : loc->cache;
  untimed(ctx);
  launch_localize_planes(map->t, R.leaf, R.min_points, R.planarity, cache, d_poses_in, (uint32_t)n_clouds, S.max_iterations, loc->state, ctx->stream);
  for (CloudChunks ch(offsets, n_clouds); ch.next();) {
    LocState* state = loc->state + ch.c0;
    for (uint32_t it = 0; it < S.max_iterations; it++) {
      launch_localize_accumulate(d_points, f32, (uint32_t)stride, ch.offs, ch.nc, ch.largest, state, R, map->t, cache, false, loc->partials, ctx->stream);
      launch_localize_step(ch.offs, ch.nc, state, S, loc->partials, false, nullptr, nullptr, nullptr, ctx->stream);
    }
    launch_localize_accumulate(d_points, f32, (uint32_t)stride, ch.offs, ch.nc, ch.largest, state, R, map->t, cache, true, loc->partials, ctx->stream);
    launch_localize_step(ch.offs, ch.nc, state, S, loc->partials, true, d_poses_out + ch.c0 * 7, reinterpret_cast<LocResult*>(d_results) + ch.c0,
                         d_info ? d_info + ch.c0 : nullptr, ctx->stream);
    CHECK_LAUNCH(ctx, "surfel localisation kernels");
  }
  return LOAMX_OK;
}

int run_dev(loamx_ctx* ctx, loamx_surfel_localizer* loc, const void* d_points, bool f32, size_t stride, const size_t* offsets, size_t n_clouds,
            const double* d_poses_in, double* d_poses_out, loamx_localize_result* d_results, loamx_reg_information* d_info,
            const loamx_localize_params* p) {
  API_ENTER(ctx);
  size_t total = 0;
  int rc = run_check(ctx, loc, d_points, stride, offsets, n_clouds, d_poses_in, d_poses_out, d_results, p, &total);
  if (rc != LOAMX_OK || n_clouds == 0) return rc;
  return run_locked(ctx, loc, d_points, f32, stride, offsets, n_clouds, d_poses_in, d_poses_out, d_results, d_info, p);
}

int run_host(loamx_ctx* ctx, loamx_surfel_localizer* loc, const void* points, bool f32, size_t stride, size_t n, const double* pose,
             const loamx_localize_params* p, loamx_localize_result* result, loamx_reg_information* info) {
  API_ENTER(ctx);
  const size_t offsets[2] = {0, n};
  size_t total = 0;
  if (!pose || !result) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  int rc = run_check(ctx, loc, points, stride, offsets, 1, pose, pose, result, p, &total);
  if (rc != LOAMX_OK) return rc;
  if (n > (~(size_t)0) / (stride * sizeof(double))) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "the cloud does not fit the address space");
  const size_t in_bytes = n * stride * (f32 ? sizeof(float) : sizeof(double));
  const size_t o_info = align256(sizeof(loamx_localize_result));
  untimed(ctx);
  ENSURE(ctx, WS_LOC_IN, in_bytes);
  ENSURE(ctx, WS_LOC_POSE, 7 * sizeof(double));
  ENSURE(ctx, WS_LOC_OUT, o_info + sizeof(loamx_reg_information));
  char* out = static_cast<char*>(ctx->ws[WS_LOC_OUT].p);
  if (in_bytes) HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[WS_LOC_IN].p, points, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[WS_LOC_POSE].p, pose, 7 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  rc = run_locked(ctx, loc, ctx->ws[WS_LOC_IN].p, f32, stride, offsets, 1, wsp<double>(ctx, WS_LOC_POSE), wsp<double>(ctx, WS_LOC_POSE),
                  reinterpret_cast<loamx_localize_result*>(out), info ? reinterpret_cast<loamx_reg_information*>(out + o_info) : nullptr, p);
  if (rc != LOAMX_OK) {
    (void)hipStreamSynchronize(ctx->stream);  // (the upload must not outlive the caller's array)
    return rc;
  }
  loamx_localize_result res;  // (the caller's records are written only when everything has arrived)
  loamx_reg_information rec;
  HIP_TRY(ctx, hipMemcpyAsync(&res, out, sizeof(res), hipMemcpyDeviceToHost, ctx->stream));
  if (info) HIP_TRY(ctx, hipMemcpyAsync(&rec, out + o_info, sizeof(rec), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *result = res;
  if (info) *info = rec;
  return LOAMX_OK;
}

}  // namespace

extern "C" {

void loamx_default_localize_params(loamx_localize_params* p) {
  if (!p) return;
  p->neighborhood = 7, p->min_points = 5, p->planarity = 0.1, p->max_distance = 0.0, p->huber_delta = 0.1;
  p->max_iterations = 10, p->min_rows = 100, p->rotation_convergence_thresh = 1e-3, p->position_convergence_thresh = 1e-2;
  p->min_eigenvalue_per_row = 1e-3;
}

int loamx_surfel_localizer_create(loamx_ctx* ctx, const loamx_surfel_map* map, size_t max_clouds, size_t max_points, loamx_surfel_localizer** out) {
  API_ENTER(ctx);
  if (!map || !out) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  *out = nullptr;
  if (map->owner != ctx) return fail(ctx, LOAMX_ERR_BAD_PARAM, "the surfel map was created on another context");
  if (max_clouds == 0) return fail(ctx, LOAMX_ERR_BAD_PARAM, "max_clouds must be >= 1");
  if (max_clouds > kLocMaxClouds) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "max_clouds > 2^24 not supported");
  if (max_points > kCloudMaxOffered) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "max_points > 2^32 - 2 not supported");
  const size_t cap = (size_t)1 << map->t.log2_cap;
  const size_t o_cache = 0, o_part = o_cache + align256(cap * sizeof(LocPlane));
  const size_t o_state = o_part + align256(localize_partials(max_points) * sizeof(LocPartial));
  const size_t bytes = o_state + align256(max_clouds * sizeof(LocState));
  loamx_surfel_localizer* loc = new loamx_surfel_localizer;
  hipError_t e = hipMalloc(&loc->block, bytes);
  if (e == hipSuccess) e = hipMemsetAsync(loc->block, 0, bytes, ctx->stream);  // (a slot never written reads as not usable)
  if (e != hipSuccess) {
    if (loc->block) (void)hipFree(loc->block);
    delete loc;
    return fail(ctx, LOAMX_ERR_HIP, std::string("localiser storage: ") + hipGetErrorString(e));
  }
  untimed(ctx);
  char* b = static_cast<char*>(loc->block);
  loc->owner = ctx, loc->device = ctx->device, loc->map = map, loc->max_clouds = max_clouds, loc->max_points = max_points;
  loc->cache = reinterpret_cast<LocPlane*>(b + o_cache), loc->partials = reinterpret_cast<LocPartial*>(b + o_part);
  loc->state = reinterpret_cast<LocState*>(b + o_state);
  *out = loc;
  return LOAMX_OK;
}

void loamx_surfel_localizer_destroy(loamx_ctx* ctx, loamx_surfel_localizer* loc) {
  if (!loc) return;
  {
    std::unique_lock<std::mutex> guard;
    if (ctx) {
      guard = std::unique_lock<std::mutex>(ctx->mu);
      (void)hipSetDevice(ctx->device);
      (void)hipStreamSynchronize(ctx->stream);
    }
    if (loc->block) (void)hipFree(loc->block);
  }
  delete loc;
}

int loamx_surfel_localizer_run(loamx_ctx* ctx, loamx_surfel_localizer* loc, const double* d_points, size_t point_stride, const size_t* cloud_offsets,
                               size_t n_clouds, const double* d_poses_in, double* d_poses_out, loamx_localize_result* d_results,
                               loamx_reg_information* d_info, const loamx_localize_params* params) {
  return run_dev(ctx, loc, d_points, false, point_stride, cloud_offsets, n_clouds, d_poses_in, d_poses_out, d_results, d_info, params);
}
int loamx_surfel_localizer_run_f32(loamx_ctx* ctx, loamx_surfel_localizer* loc, const float* d_points, size_t point_stride, const size_t* cloud_offsets,
                                   size_t n_clouds, const double* d_poses_in, double* d_poses_out, loamx_localize_result* d_results,
                                   loamx_reg_information* d_info, const loamx_localize_params* params) {
  return run_dev(ctx, loc, d_points, true, point_stride, cloud_offsets, n_clouds, d_poses_in, d_poses_out, d_results, d_info, params);
}
int loamx_surfel_localizer_run_host(loamx_ctx* ctx, loamx_surfel_localizer* loc, const double* points, size_t point_stride, size_t n_points,
                                    const double pose[7], const loamx_localize_params* params, loamx_localize_result* result,
                                    loamx_reg_information* info) {
  return run_host(ctx, loc, points, false, point_stride, n_points, pose, params, result, info);
}
int loamx_surfel_localizer_run_host_f32(loamx_ctx* ctx, loamx_surfel_localizer* loc, const float* points, size_t point_stride, size_t n_points,
                                        const double pose[7], const loamx_localize_params* params, loamx_localize_result* result,
                                        loamx_reg_information* info) {
  return run_host(ctx, loc, points, true, point_stride, n_points, pose, params, result, info);
}

}  // extern "C"
