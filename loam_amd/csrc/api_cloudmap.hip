// api_cloudmap.hip — the cloud map (loamx.h, "cloud map"): the map handle with its one device block (table, voxel list, counters,
// the scratch of a round of launches), the add, emit, clear and stats entry points and their host forms.
#include "api_voxelmap.h"
#include "cloudmap_math.h"

struct loamx_cloud_map : loamx::VoxelMapBase {  // ones: keys + first; zeros: sums, count, counters and lengths
  loamx_cloud_map_params params = {};
  loamx::CloudRule rule = {};
  loamx::CloudTable t = {};
  uint32_t* d_slot = nullptr;   // scratch of a round of an add: [kCloudChunkPoints]
  uint8_t* d_keep = nullptr;    // [max(kCloudChunkPoints, max_voxels)] (add and emit)
  uint32_t* d_tiles = nullptr;  // the compaction's tiles for as many
};

using namespace loamx;

namespace {

constexpr size_t kCloudMaxVoxels = (size_t)1 << 30;

// the clouds of the call chunk by chunk, their points in rounds of kCloudChunkPoints; `offered` is the running index of the call's
// first point
int add_locked(loamx_ctx* ctx, VoxelMapBase* base, const void* d_points, bool f32, size_t stride, const size_t* offsets, size_t n_clouds,
               const double* d_poses) {
  loamx_cloud_map* map = static_cast<loamx_cloud_map*>(base);
  const bool combine = !(ctx->reg_flags & kRegFlagNoCloudmapCombine);
  const double point_bytes = f32 ? 12.0 : 24.0;
  for (CloudChunks ch(offsets, n_clouds); ch.next();) {
    for (unsigned long long p0 = ch.offs.off[0]; p0 < ch.offs.off[ch.nc]; p0 += kCloudChunkPoints) {
      const uint32_t n = (uint32_t)(ch.offs.off[ch.nc] - p0 < kCloudChunkPoints ? ch.offs.off[ch.nc] - p0 : kCloudChunkPoints);
      const uint32_t g0 = (uint32_t)(map->offered + (p0 - offsets[0]));
      {
        TimedScope timed(ctx, combine ? LOAMX_K_CLOUD_ACCUMULATE : LOAMX_K_CLOUD_ACCUMULATE_PLAIN, point_bytes * n, true);
        launch_cloud_accumulate(d_points, f32, (uint32_t)stride, ch.offs, ch.nc, p0, n, g0, d_poses ? d_poses + ch.c0 * 7 : nullptr, map->rule, map->t,
                                combine, map->d_slot, ctx->stream);
      }
      {
        TimedScope timed(ctx, LOAMX_K_CLOUD_LIST, 5.0 * n, true);
        launch_cloud_list(map->t, map->d_slot, n, g0, map->d_keep, map->d_tiles, ctx->stream);
      }
      CHECK_LAUNCH(ctx, "cloud map add kernels");
    }
  }
  map->offered += offsets[n_clouds] - offsets[0];
  return LOAMX_OK;
}

const VoxelMapKind kKind = {"cloud map", "a cloud map", "points", kCloudMaxOffered, WS_CLOUD_IN, WS_CLOUD_POSE, add_locked};

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
  API_ENTER(ctx);
  if (!params || !out) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  *out = nullptr;
  if (!isfinite(params->leaf) || !(params->leaf > 0.0)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "leaf must be finite and positive");
  if (!isfinite(params->min_range) || params->min_range < 0.0) return fail(ctx, LOAMX_ERR_BAD_PARAM, "min_range must be finite and not negative");
  if (!(params->max_range >= params->min_range)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "max_range must be at least min_range");
  if (max_voxels == 0) return fail(ctx, LOAMX_ERR_BAD_PARAM, "max_voxels must be >= 1");
  if (max_voxels > kCloudMaxVoxels) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "max_voxels > 2^30 not supported");
  loamx_cloud_map* map = new loamx_cloud_map;
  map->owner = ctx, map->device = ctx->device;
  map->params = *params;
  map->rule.leaf = params->leaf;
  map->rule.min_r2 = params->min_range * params->min_range, map->rule.max_r2 = params->max_range * params->max_range;
  const uint32_t log2_cap = voxel_table_log2(2 * max_voxels);
  const size_t cap = (size_t)1 << log2_cap, scratch = max_voxels > kCloudChunkPoints ? max_voxels : kCloudChunkPoints;
  const size_t o_keys = 0, o_first = o_keys + align256(cap * sizeof(unsigned long long));
  const size_t o_sums = o_first + align256(cap * sizeof(uint32_t)), o_count = o_sums + align256(cap * 3 * sizeof(unsigned long long));
  const size_t o_words = o_count + align256(cap * sizeof(uint32_t)), o_lens = o_words + align256(kCloudWords * sizeof(unsigned long long));
  const size_t o_list = o_lens + align256(kCloudLens * sizeof(uint32_t)), o_slot = o_list + align256(max_voxels * sizeof(uint32_t));
  const size_t o_keep = o_slot + align256((size_t)kCloudChunkPoints * sizeof(uint32_t)), o_tiles = o_keep + align256(scratch);
  const size_t bytes = o_tiles + align256(map_compact_ws_bytes(scratch));
  hipError_t e = hipMalloc(&map->block, bytes);
  if (e != hipSuccess) {
    delete map;
    return fail(ctx, LOAMX_ERR_HIP, std::string("cloud map storage: ") + hipGetErrorString(e));
  }
  char* b = static_cast<char*>(map->block);
  map->ones_bytes = o_sums, map->zeros_bytes = o_list - o_sums;
  map->t.keys = reinterpret_cast<unsigned long long*>(b + o_keys), map->t.first = reinterpret_cast<uint32_t*>(b + o_first);
  map->t.sums = reinterpret_cast<unsigned long long*>(b + o_sums), map->t.count = reinterpret_cast<uint32_t*>(b + o_count);
  map->t.words = reinterpret_cast<unsigned long long*>(b + o_words), map->t.lens = reinterpret_cast<uint32_t*>(b + o_lens);
  map->t.list = reinterpret_cast<uint32_t*>(b + o_list);
  map->t.log2_cap = log2_cap, map->t.max_voxels = (uint32_t)max_voxels;
  map->d_slot = reinterpret_cast<uint32_t*>(b + o_slot), map->d_keep = reinterpret_cast<uint8_t*>(b + o_keep);
  map->d_tiles = reinterpret_cast<uint32_t*>(b + o_tiles);
  int rc = voxel_map_clear(ctx, map);
  if (rc != LOAMX_OK) {
    (void)hipFree(map->block);
    delete map;
    return rc;
  }
  *out = map;
  return LOAMX_OK;
}

void loamx_cloud_map_destroy(loamx_ctx* ctx, loamx_cloud_map* map) {
  if (!map) return;
  voxel_map_destroy(ctx, map);
  delete map;
}

int loamx_cloud_map_clear(loamx_ctx* ctx, loamx_cloud_map* map) {
  API_ENTER(ctx);
  int rc = voxel_map_check(ctx, map, kKind);
  if (rc != LOAMX_OK) return rc;
  return voxel_map_clear(ctx, map);
}

int loamx_cloud_map_crop(loamx_ctx* ctx, loamx_cloud_map* map, const double* d_pose, const double lo[3], const double hi[3], uint32_t* d_counts_out) {
  CropTable t = {};
  if (map)
    t = {map->t.keys, map->t.sums, map->t.first, map->t.count, map->t.list, map->t.lens + kCloudLenListed, nullptr, map->t.log2_cap, 3u, map->t.max_voxels};
  return voxel_map_crop(ctx, map, kKind, t, map ? map->rule.leaf : 0.0, d_pose, lo, hi, d_counts_out);
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
  untimed(ctx);
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_pinned, b + o_n, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  const size_t n = ctx->h_pinned[0], m = n < capacity ? n : capacity;
  if (m) {
    HIP_TRY(ctx, hipMemcpyAsync(xyz_out, b, m * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (count_out) HIP_TRY(ctx, hipMemcpyAsync(count_out, b + o_count, m * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (first_out) HIP_TRY(ctx, hipMemcpyAsync(first_out, b + o_first, m * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  *n_out = n;
  return LOAMX_OK;
}

int loamx_cloud_map_stats_read(loamx_ctx* ctx, const loamx_cloud_map* map, loamx_cloud_map_stats* out) {
  API_ENTER(ctx);
  int rc = voxel_map_check(ctx, map, kKind);
  if (rc != LOAMX_OK) return rc;
  if (!out) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  unsigned long long words[kCloudWords];
  uint32_t lens[kCloudLens];
  untimed(ctx);
  HIP_TRY(ctx, hipMemcpyAsync(words, map->t.words, sizeof(words), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(lens, map->t.lens, sizeof(lens), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  out->voxels = lens[kCloudLenListed], out->points_offered = map->offered;
  out->points_used = words[kCloudUsed], out->invalid = words[kCloudInvalid], out->range = words[kCloudRange];
  out->outside = words[kCloudOutside], out->overflow = words[kCloudWordOverflow];
  return LOAMX_OK;
}

int loamx_cloud_map_claims_read(loamx_ctx* ctx, const loamx_cloud_map* map, uint64_t* claims) {
  return voxel_map_read_word(ctx, map, kKind, map ? map->t.words + kCloudWordClaims : nullptr, claims);
}

}  // extern "C"
