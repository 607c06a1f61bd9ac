// api_surfel.hip — the surfel map (loamx.h, "surfel map"): the map handle with its one device block (table, voxel list, counters,
// the scratch of a round of launches), the add, emit, query, clear and stats entry points and their host forms. On this handle
// the plain names are the device forms.
#include "api_surfel.h"
#include "surfel_math.h"

using namespace loamx;

namespace {

static_assert(sizeof(loamx_surfel) == 128, "loamx_surfel is 128 bytes");
constexpr size_t kSurfelMaxVoxels = (size_t)1 << 30;
constexpr size_t kSurfelMaxQuery = (size_t)1 << 31;

// the clouds of the call chunk by chunk, their points in rounds of kCloudChunkPoints (the cloud map's add_locked)
int add_locked(loamx_ctx* ctx, VoxelMapBase* base, const void* d_points, bool f32, size_t stride, const size_t* offsets, size_t n_clouds,
               const double* d_poses) {
  loamx_surfel_map* map = static_cast<loamx_surfel_map*>(base);
  const bool combine = !(ctx->reg_flags & kRegFlagNoSurfelCombine);
  untimed(ctx);
  for (CloudChunks ch(offsets, n_clouds); ch.next();) {
    for (unsigned long long p0 = ch.offs.off[0]; p0 < ch.offs.off[ch.nc]; p0 += kCloudChunkPoints) {
      const uint32_t n = (uint32_t)(ch.offs.off[ch.nc] - p0 < kCloudChunkPoints ? ch.offs.off[ch.nc] - p0 : kCloudChunkPoints);
      const uint32_t g0 = (uint32_t)(map->offered + (p0 - offsets[0]));
      launch_surfel_accumulate(d_points, f32, (uint32_t)stride, ch.offs, ch.nc, p0, n, g0, d_poses ? d_poses + ch.c0 * 7 : nullptr, map->rule, map->t,
                               combine, map->d_slot, ctx->stream);
      launch_surfel_list(map->t, map->d_slot, n, g0, map->d_keep, map->d_tiles, ctx->stream);
      CHECK_LAUNCH(ctx, "surfel map add kernels");
    }
  }
  map->offered += offsets[n_clouds] - offsets[0];
  return LOAMX_OK;
}

const VoxelMapKind kKind = {"surfel map", "a surfel map", "points", kCloudMaxOffered, WS_SURFEL_IN, WS_SURFEL_POSE, add_locked};

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
  API_ENTER(ctx);
  if (!params || !out) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  *out = nullptr;
  if (!isfinite(params->leaf) || !(params->leaf > 0.0)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "leaf must be finite and positive");
  if (!isfinite(params->min_range) || params->min_range < 0.0) return fail(ctx, LOAMX_ERR_BAD_PARAM, "min_range must be finite and not negative");
  if (!(params->max_range >= params->min_range)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "max_range must be at least min_range");
  if (max_voxels == 0) return fail(ctx, LOAMX_ERR_BAD_PARAM, "max_voxels must be >= 1");
  if (max_voxels > kSurfelMaxVoxels) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "max_voxels > 2^30 not supported");
  loamx_surfel_map* map = new loamx_surfel_map;
  map->owner = ctx, map->device = ctx->device;
  map->params = *params;
  map->rule.leaf = params->leaf;
  map->rule.min_r2 = params->min_range * params->min_range, map->rule.max_r2 = params->max_range * params->max_range;
  const uint32_t log2_cap = voxel_table_log2(2 * max_voxels);
  const size_t cap = (size_t)1 << log2_cap, scratch = max_voxels > kCloudChunkPoints ? max_voxels : kCloudChunkPoints;
  const size_t o_keys = 0, o_first = o_keys + align256(cap * sizeof(unsigned long long));
  const size_t o_mom = o_first + align256(cap * sizeof(uint32_t)), o_count = o_mom + align256(cap * kSurfelSlotWords * sizeof(unsigned long long));
  const size_t o_words = o_count + align256(cap * sizeof(uint32_t)), o_lens = o_words + align256(kCloudWords * sizeof(unsigned long long));
  const size_t o_list = o_lens + align256(kCloudLens * sizeof(uint32_t)), o_slot = o_list + align256(max_voxels * sizeof(uint32_t));
  const size_t o_keep = o_slot + align256((size_t)kCloudChunkPoints * sizeof(uint32_t)), o_tiles = o_keep + align256(scratch);
  const size_t bytes = o_tiles + align256(map_compact_ws_bytes(scratch));
  hipError_t e = hipMalloc(&map->block, bytes);
  if (e != hipSuccess) {
    delete map;
    return fail(ctx, LOAMX_ERR_HIP, std::string("surfel map storage: ") + hipGetErrorString(e));
  }
  char* b = static_cast<char*>(map->block);
  map->ones_bytes = o_mom, map->zeros_bytes = o_list - o_mom;
  map->t.keys = reinterpret_cast<unsigned long long*>(b + o_keys), map->t.first = reinterpret_cast<uint32_t*>(b + o_first);
  map->t.mom = reinterpret_cast<unsigned long long*>(b + o_mom), map->t.count = reinterpret_cast<uint32_t*>(b + o_count);
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

void loamx_surfel_map_destroy(loamx_ctx* ctx, loamx_surfel_map* map) {
  if (!map) return;
  voxel_map_destroy(ctx, map);
  delete map;
}

int loamx_surfel_map_clear(loamx_ctx* ctx, loamx_surfel_map* map) {
  API_ENTER(ctx);
  int rc = voxel_map_check(ctx, map, kKind);
  if (rc != LOAMX_OK) return rc;
  return voxel_map_clear(ctx, map);
}

int loamx_surfel_map_crop(loamx_ctx* ctx, loamx_surfel_map* map, const double* d_pose, const double lo[3], const double hi[3], uint32_t* d_counts_out) {
  CropTable t = {};
  if (map)
    t = {map->t.keys, map->t.mom, map->t.first, map->t.count, map->t.list, map->t.lens + kCloudLenListed, nullptr, map->t.log2_cap, kSurfelSlotWords,
         map->t.max_voxels};
  return voxel_map_crop(ctx, map, kKind, t, map ? map->rule.leaf : 0.0, d_pose, lo, hi, d_counts_out);
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
  untimed(ctx);
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_pinned, b + o_n, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  const size_t n = ctx->h_pinned[0], m = n < capacity ? n : capacity;
  if (m) {
    HIP_TRY(ctx, hipMemcpyAsync(out, b, m * sizeof(loamx_surfel), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  *n_out = n;
  return LOAMX_OK;
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

int loamx_surfel_map_claims_read(loamx_ctx* ctx, const loamx_surfel_map* map, uint64_t* claims) {
  return voxel_map_read_word(ctx, map, kKind, map ? map->t.words + kCloudWordClaims : nullptr, claims);
}

}  // extern "C"
