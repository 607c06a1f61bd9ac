// api_surfel.hip — the surfel map (loamx.h, "surfel map"): the entry points of the handle. What it shares with the cloud map is in
// api_listedmap.h; its own are the emit of records with its host form and the query. Nothing of it is timed. On this handle the plain
// names are the device forms.
#include "api_listedmap.h"
#include "surfel_math.h"

using namespace loamx;

namespace {

static_assert(sizeof(loamx_surfel) == 128, "loamx_surfel is 128 bytes");
constexpr size_t kSurfelMaxQuery = (size_t)1 << 31;

const ListedMapKind kKind = {{"surfel map", "a surfel map", "points", kCloudMaxOffered, WS_SURFEL_IN, WS_SURFEL_POSE, listed_map_add_locked},
                             kSurfelSlotWords, launch_surfel_accumulate, kRegFlagNoSurfelCombine, -1, -1, -1};

int emit_check(loamx_ctx* ctx, const loamx_surfel_map* map, const void* n_out) {
  int rc = voxel_map_check(ctx, map, kKind);
  if (rc != LOAMX_OK) return rc;
  if (!n_out) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  return LOAMX_OK;
}

int emit_locked(loamx_ctx* ctx, const loamx_surfel_map* map, uint32_t min_points, loamx_surfel* d_out, double* d_xyz, double* d_normal, size_t capacity,
                uint32_t* d_n_out) {
  untimed(ctx);
  launch_surfel_emit(map->t, map->rule.leaf, min_points, map->d_keep, map->d_tiles, d_out, d_xyz, d_normal, capacity, d_n_out, ctx->stream);
  CHECK_LAUNCH(ctx, "surfel map emit kernels");
  return LOAMX_OK;
}

}  // namespace

extern "C" {

void loamx_default_surfel_map_params(loamx_surfel_map_params* p) {
  if (!p) return;
  p->leaf = 0.5, p->min_range = 0.5, p->max_range = 120.0;
}

int loamx_surfel_map_create(loamx_ctx* ctx, const loamx_surfel_map_params* params, size_t max_voxels, loamx_surfel_map** out) {
  return listed_map_create(ctx, kKind, params, max_voxels, out);
}
void loamx_surfel_map_destroy(loamx_ctx* ctx, loamx_surfel_map* map) { listed_map_destroy(ctx, map); }
int loamx_surfel_map_clear(loamx_ctx* ctx, loamx_surfel_map* map) { return listed_map_clear(ctx, map, kKind); }
int loamx_surfel_map_crop(loamx_ctx* ctx, loamx_surfel_map* map, const double* d_pose, const double lo[3], const double hi[3], uint32_t* d_counts_out) {
  return listed_map_crop(ctx, map, kKind, d_pose, lo, hi, d_counts_out);
}

int loamx_surfel_map_add_clouds(loamx_ctx* ctx, loamx_surfel_map* map, const double* d_points, size_t point_stride, const size_t* cloud_offsets,
                                size_t n_clouds, const double* d_poses) {
  return voxel_map_add_dev(ctx, map, kKind, d_points, false, point_stride, cloud_offsets, n_clouds, d_poses);
}
int loamx_surfel_map_add_clouds_f32(loamx_ctx* ctx, loamx_surfel_map* map, const float* d_points, size_t point_stride, const size_t* cloud_offsets,
                                    size_t n_clouds, const double* d_poses) {
  return voxel_map_add_dev(ctx, map, kKind, d_points, true, point_stride, cloud_offsets, n_clouds, d_poses);
}
int loamx_surfel_map_add_cloud_host(loamx_ctx* ctx, loamx_surfel_map* map, const double* points, size_t point_stride, size_t n_points,
                                    const double pose[7]) {
  return voxel_map_add_host(ctx, map, kKind, points, false, point_stride, n_points, pose);
}
int loamx_surfel_map_add_cloud_host_f32(loamx_ctx* ctx, loamx_surfel_map* map, const float* points, size_t point_stride, size_t n_points,
                                        const double pose[7]) {
  return voxel_map_add_host(ctx, map, kKind, points, true, point_stride, n_points, pose);
}

int loamx_surfel_map_emit(loamx_ctx* ctx, const loamx_surfel_map* map, uint32_t min_points, loamx_surfel* d_out, double* d_xyz_out,
                          double* d_normal_out, size_t capacity, uint32_t* d_n_out) {
  API_ENTER(ctx);
  int rc = emit_check(ctx, map, d_n_out);
  if (rc != LOAMX_OK) return rc;
  return emit_locked(ctx, map, min_points, d_out, d_xyz_out, d_normal_out, capacity, d_n_out);
}

int loamx_surfel_map_emit_host(loamx_ctx* ctx, const loamx_surfel_map* map, uint32_t min_points, loamx_surfel* out, size_t capacity, size_t* n_out) {
  API_ENTER(ctx);
  int rc = emit_check(ctx, map, n_out);
  if (rc != LOAMX_OK) return rc;
  if (capacity && !out) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  if (capacity > map->t.max_voxels) capacity = map->t.max_voxels;  // (no more can qualify)
  const size_t o_n = align256(capacity * sizeof(loamx_surfel));
  untimed(ctx);
  ENSURE(ctx, WS_SURFEL_OUT, o_n + 256);
  char* b = static_cast<char*>(ctx->ws[WS_SURFEL_OUT].p);
  rc = emit_locked(ctx, map, min_points, reinterpret_cast<loamx_surfel*>(b), nullptr, nullptr, capacity, reinterpret_cast<uint32_t*>(b + o_n));
  if (rc != LOAMX_OK) return rc;
  const EmitCopy copy = {out, b, sizeof(loamx_surfel)};
  return listed_emit_read(ctx, b + o_n, capacity, &copy, 1, n_out);
}

int loamx_surfel_map_query(loamx_ctx* ctx, const loamx_surfel_map* map, const double* d_points, size_t point_stride, size_t n_points,
                           uint32_t min_points, loamx_surfel* d_out, double* d_distance_out, uint32_t* d_count_out) {
  API_ENTER(ctx);
  int rc = voxel_map_check(ctx, map, kKind);
  if (rc != LOAMX_OK) return rc;
  if (point_stride < 3) return fail(ctx, LOAMX_ERR_BAD_PARAM, "point_stride must be >= 3");
  if (point_stride > 0xFFFFFFFFull) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "point_stride does not fit 32 bits");
  if (n_points && !d_points) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null points");
  if (n_points > kSurfelMaxQuery) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "more than 2^31 points in one query");
  untimed(ctx);
  launch_surfel_query(map->t, map->rule.leaf, min_points, d_points, (uint32_t)point_stride, n_points, d_out, d_distance_out, d_count_out, ctx->stream);
  CHECK_LAUNCH(ctx, "surfel map query kernel");
  return LOAMX_OK;
}

int loamx_surfel_map_stats_read(loamx_ctx* ctx, const loamx_surfel_map* map, loamx_surfel_map_stats* out) {
  return listed_map_stats_read(ctx, map, kKind, out);
}
int loamx_surfel_map_claims_read(loamx_ctx* ctx, const loamx_surfel_map* map, uint64_t* claims) { return listed_map_claims_read(ctx, map, kKind, claims); }

}  // extern "C"
