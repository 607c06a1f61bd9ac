// api_cloudmap.hip — the cloud map (loamx.h, "cloud map"): the entry points of the handle. What it shares with the surfel map is
// in api_listedmap.h; its own are the timed rows of its add and the emit of centroids with its host form.
#include "api_listedmap.h"
#include "cloudmap_math.h"

using namespace loamx;

namespace {

const ListedMapKind kKind = {{"cloud map", "a cloud map", "points", kCloudMaxOffered, WS_CLOUD_IN, WS_CLOUD_POSE, listed_map_add_locked},
                             kCloudSlotWords, launch_cloud_accumulate, kRegFlagNoCloudmapCombine,
                             LOAMX_K_CLOUD_ACCUMULATE, LOAMX_K_CLOUD_ACCUMULATE_PLAIN, LOAMX_K_CLOUD_LIST};

int emit_check(loamx_ctx* ctx, const loamx_cloud_map* map, const void* xyz, size_t capacity, const void* n_out) {
  int rc = voxel_map_check(ctx, map, kKind);
  if (rc != LOAMX_OK) return rc;
  if (!n_out || (capacity && !xyz)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  return LOAMX_OK;
}

int emit_locked(loamx_ctx* ctx, const loamx_cloud_map* map, uint32_t min_points, double* d_xyz, uint32_t* d_count, uint32_t* d_first, size_t capacity,
                uint32_t* d_n_out) {
  TimedScope timed(ctx, LOAMX_K_CLOUD_EMIT, 0.0, true);
  launch_cloud_emit(map->t, map->rule.leaf, min_points, map->d_keep, map->d_tiles, d_xyz, d_count, d_first, capacity, d_n_out, ctx->stream);
  CHECK_LAUNCH(ctx, "cloud map emit kernels");
  return LOAMX_OK;
}

}  // namespace

extern "C" {

void loamx_default_cloud_map_params(loamx_cloud_map_params* p) {
  if (!p) return;
  p->leaf = 0.2, p->min_range = 0.5, p->max_range = 120.0;
}

int loamx_cloud_map_create(loamx_ctx* ctx, const loamx_cloud_map_params* params, size_t max_voxels, loamx_cloud_map** out) {
  return listed_map_create(ctx, kKind, params, max_voxels, out);
}
void loamx_cloud_map_destroy(loamx_ctx* ctx, loamx_cloud_map* map) { listed_map_destroy(ctx, map); }
int loamx_cloud_map_clear(loamx_ctx* ctx, loamx_cloud_map* map) { return listed_map_clear(ctx, map, kKind); }
int loamx_cloud_map_crop(loamx_ctx* ctx, loamx_cloud_map* map, const double* d_pose, const double lo[3], const double hi[3], uint32_t* d_counts_out) {
  return listed_map_crop(ctx, map, kKind, d_pose, lo, hi, d_counts_out);
}

int loamx_cloud_map_add_clouds_dev(loamx_ctx* ctx, loamx_cloud_map* map, const double* d_points, size_t point_stride, const size_t* cloud_offsets,
                                   size_t n_clouds, const double* d_poses) {
  return voxel_map_add_dev(ctx, map, kKind, d_points, false, point_stride, cloud_offsets, n_clouds, d_poses);
}
int loamx_cloud_map_add_clouds_dev_f32(loamx_ctx* ctx, loamx_cloud_map* map, const float* d_points, size_t point_stride, const size_t* cloud_offsets,
                                       size_t n_clouds, const double* d_poses) {
  return voxel_map_add_dev(ctx, map, kKind, d_points, true, point_stride, cloud_offsets, n_clouds, d_poses);
}
int loamx_cloud_map_add_cloud(loamx_ctx* ctx, loamx_cloud_map* map, const double* points, size_t point_stride, size_t n_points, const double pose[7]) {
  return voxel_map_add_host(ctx, map, kKind, points, false, point_stride, n_points, pose);
}
int loamx_cloud_map_add_cloud_f32(loamx_ctx* ctx, loamx_cloud_map* map, const float* points, size_t point_stride, size_t n_points,
                                  const double pose[7]) {
  return voxel_map_add_host(ctx, map, kKind, points, true, point_stride, n_points, pose);
}

int loamx_cloud_map_emit_dev(loamx_ctx* ctx, const loamx_cloud_map* map, uint32_t min_points, double* d_xyz_out, uint32_t* d_count_out,
                             uint32_t* d_first_out, size_t capacity, uint32_t* d_n_out) {
  API_ENTER(ctx);
  int rc = emit_check(ctx, map, d_xyz_out, capacity, d_n_out);
  if (rc != LOAMX_OK) return rc;
  return emit_locked(ctx, map, min_points, d_xyz_out, d_count_out, d_first_out, capacity, d_n_out);
}

int loamx_cloud_map_emit(loamx_ctx* ctx, const loamx_cloud_map* map, uint32_t min_points, double* xyz_out, uint32_t* count_out, uint32_t* first_out,
                         size_t capacity, size_t* n_out) {
  API_ENTER(ctx);
  int rc = emit_check(ctx, map, xyz_out, capacity, n_out);
  if (rc != LOAMX_OK) return rc;
  if (capacity > map->t.max_voxels) capacity = map->t.max_voxels;  // (no more can qualify)
  const size_t o_count = align256(capacity * 3 * sizeof(double)), o_first = o_count + align256(capacity * sizeof(uint32_t));
  const size_t o_n = o_first + align256(capacity * sizeof(uint32_t));
  untimed(ctx);
  ENSURE(ctx, WS_CLOUD_OUT, o_n + 256);
  char* b = static_cast<char*>(ctx->ws[WS_CLOUD_OUT].p);
  rc = emit_locked(ctx, map, min_points, reinterpret_cast<double*>(b), reinterpret_cast<uint32_t*>(b + o_count), reinterpret_cast<uint32_t*>(b + o_first),
                   capacity, reinterpret_cast<uint32_t*>(b + o_n));
  if (rc != LOAMX_OK) return rc;
  const EmitCopy copies[3] = {{xyz_out, b, 3 * sizeof(double)}, {count_out, b + o_count, sizeof(uint32_t)}, {first_out, b + o_first, sizeof(uint32_t)}};
  return listed_emit_read(ctx, b + o_n, capacity, copies, 3, n_out);
}

int loamx_cloud_map_stats_read(loamx_ctx* ctx, const loamx_cloud_map* map, loamx_cloud_map_stats* out) {
  return listed_map_stats_read(ctx, map, kKind, out);
}
int loamx_cloud_map_claims_read(loamx_ctx* ctx, const loamx_cloud_map* map, uint64_t* claims) { return listed_map_claims_read(ctx, map, kKind, claims); }

}  // extern "C"
