// api_occupancy.hip — the occupancy map (loamx.h, "occupancy map"): the map handle with its one device block (table and counters),
// the add, clear, query, box, slice and stats entry points and their host forms, and the distance field of a box or slice
// (loamx.h, "occupancy distance field") with the staging the handle keeps for it.
#include "api_occupancy.h"
#include "distance_math.h"

using namespace loamx;

namespace {

constexpr size_t kOccMaxVoxels = (size_t)1 << 30;
constexpr unsigned long long kOccMaxRead = 1ull << 31;  // points of a query, voxels of a box

// the clouds of the call chunk by chunk, their rays in launches of kOccChunkRays
int add_locked(loamx_ctx* ctx, VoxelMapBase* base, const VoxelMapKind&, const void* d_points, bool f32, size_t stride, const size_t* offsets, size_t n_clouds,
               const double* d_poses) {
  loamx_occupancy_map* map = static_cast<loamx_occupancy_map*>(base);
  const bool combine = !(ctx->reg_flags & kRegFlagNoOccupancyCombine);
  untimed(ctx);
  for (CloudChunks ch(offsets, n_clouds); ch.next();) {
    for (unsigned long long p0 = ch.offs.off[0]; p0 < ch.offs.off[ch.nc]; p0 += kOccChunkRays) {
      const uint32_t n = (uint32_t)(ch.offs.off[ch.nc] - p0 < kOccChunkRays ? ch.offs.off[ch.nc] - p0 : kOccChunkRays);
      launch_occupancy_walk(d_points, f32, (uint32_t)stride, ch.offs, ch.nc, p0, n, d_poses ? d_poses + ch.c0 * 7 : nullptr, map->rule, map->t, combine,
                            ctx->stream);
      CHECK_LAUNCH(ctx, "occupancy walk kernel");
    }
  }
  map->offered += offsets[n_clouds] - offsets[0];
  return LOAMX_OK;
}

const VoxelMapKind kKind = {"occupancy map", "an occupancy map", "rays", kOccMaxOffered, WS_OCC_IN, WS_OCC_POSE, add_locked};

int query_check(loamx_ctx* ctx, const loamx_occupancy_map* map, const void* points, size_t stride, size_t n) {
  int rc = voxel_map_check(ctx, map, kKind);
  if (rc != LOAMX_OK) return rc;
  if (stride < 3) return fail(ctx, LOAMX_ERR_BAD_PARAM, "point_stride must be >= 3");
  if (stride > 0xFFFFFFFFull) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "point_stride does not fit 32 bits");
  if (n && !points) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null points");
  if (n > kOccMaxRead) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "a query takes at most 2^31 points");
  return LOAMX_OK;
}

// *n: the voxels of the box (with_levels) or the columns of the slice
int box_check(loamx_ctx* ctx, const loamx_occupancy_map* map, const int32_t* vmin, const uint32_t* dims, bool with_levels, unsigned long long* n) {
  int rc = voxel_map_check(ctx, map, kKind);
  if (rc != LOAMX_OK) return rc;
  if (!vmin || !dims) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  const unsigned long long plane = (unsigned long long)dims[0] * dims[1];
  if (plane > kOccMaxRead || plane * (dims[2] ? dims[2] : 1u) > kOccMaxRead) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "a box holds at most 2^31 voxels");
  *n = with_levels ? plane * dims[2] : plane;
  return LOAMX_OK;
}

OccBox make_box(const int32_t* vmin, const uint32_t* dims) {
  OccBox b;
  for (int a = 0; a < 3; a++) b.vmin[a] = vmin[a], b.dims[a] = dims[a];
  return b;
}

int launch_box(loamx_ctx* ctx, const loamx_occupancy_map* map, const int32_t* vmin, const uint32_t* dims, uint32_t* d_counts, uint8_t* d_state) {
  untimed(ctx);
  launch_occupancy_box(map->t, map->state_rule, make_box(vmin, dims), d_counts, d_state, ctx->stream);
  CHECK_LAUNCH(ctx, "occupancy box kernel");
  return LOAMX_OK;
}

int launch_slice(loamx_ctx* ctx, const loamx_occupancy_map* map, const int32_t* vmin, const uint32_t* dims, uint8_t* d_grid) {
  untimed(ctx);
  launch_occupancy_slice(map->t, map->state_rule, make_box(vmin, dims), d_grid, ctx->stream);
  CHECK_LAUNCH(ctx, "occupancy slice kernel");
  return LOAMX_OK;
}

// counts (n x 2 words) and states (n bytes) of the workspace's output block to the host arrays that were asked for
int read_out(loamx_ctx* ctx, size_t n, uint32_t* counts_out, uint8_t* state_out) {
  char* b = static_cast<char*>(ctx->ws[WS_OCC_OUT].p);
  if (counts_out) HIP_TRY(ctx, hipMemcpyAsync(counts_out, b, n * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (state_out) HIP_TRY(ctx, hipMemcpyAsync(state_out, b + align256(n * 2 * sizeof(uint32_t)), n, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LOAMX_OK;
}

bool bad_double(double v) { return !isfinite(v) || v < 0.0; }

// the checks of a distance call; *n: the voxels of the box or the columns of the slice (0: nothing to do)
int distance_check(loamx_ctx* ctx, const loamx_occupancy_map* map, const int32_t* vmin, const uint32_t* dims, const loamx_distance_params* params,
                   bool slice, unsigned long long* n) {
  int rc = voxel_map_check(ctx, map, kKind);
  if (rc != LOAMX_OK) return rc;
  if (!vmin || !dims || !params) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  if (params->max_dist_voxels == 0) return fail(ctx, LOAMX_ERR_BAD_PARAM, "max_dist_voxels must be >= 1");
  if (params->max_dist_voxels > kDistMaxR) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "max_dist_voxels > 255 not supported");
  const unsigned long long halo = 2ull * params->max_dist_voxels;
  unsigned long long ext = dims[0] + halo;  // every factor and every product is tested before the next is formed
  if (ext <= kOccMaxRead) ext *= dims[1] + halo;
  if (ext <= kOccMaxRead && !slice) ext *= dims[2] + halo;
  if (ext > kOccMaxRead) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "the box extended by max_dist_voxels on every side holds at most 2^31 voxels");
  *n = (unsigned long long)dims[0] * dims[1] * (slice ? 1u : dims[2]);
  return LOAMX_OK;
}

// grows the handle's staging to the call's size (the only part of a distance call that may wait) and enqueues the launches
int launch_distance_call(loamx_ctx* ctx, loamx_occupancy_map* map, const int32_t* vmin, const uint32_t* dims, const loamx_distance_params* params,
                         bool slice, uint16_t* d_d2, int16_t* d_offset, float* d_metres) {
  const DistGeom g = make_dist_geom(vmin, dims, params->max_dist_voxels, params->unknown_is_obstacle != 0, slice);
  size_t bytes = 0;
  (void)dist_staging_carve(nullptr, g, &bytes);
  if (bytes > map->dist_bytes) {
    if (map->dist_block) {
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      HIP_TRY(ctx, hipFree(map->dist_block));
      map->dist_block = nullptr, map->dist_bytes = 0;
    }
    hipError_t e = hipMalloc(&map->dist_block, bytes);
    if (e != hipSuccess) {
      map->dist_block = nullptr;
      return fail(ctx, LOAMX_ERR_HIP, std::string("distance field staging: ") + hipGetErrorString(e));
    }
    map->dist_bytes = bytes;
  }
  untimed(ctx);
  launch_distance(map->t, map->state_rule, map->rule.leaf, g, dist_staging_carve(map->dist_block, g, nullptr),
                  !(ctx->reg_flags & kRegFlagNoDistanceEarlyExit), d_d2, d_offset, d_metres, ctx->stream);
  CHECK_LAUNCH(ctx, "occupancy distance kernels");
  return LOAMX_OK;
}

int distance_dev(loamx_ctx* ctx, loamx_occupancy_map* map, const int32_t* vmin, const uint32_t* dims, const loamx_distance_params* params, bool slice,
                 uint16_t* d_d2, int16_t* d_offset, float* d_metres) {
  API_ENTER(ctx);
  unsigned long long n = 0;
  int rc = distance_check(ctx, map, vmin, dims, params, slice, &n);
  if (rc != LOAMX_OK || n == 0 || (!d_d2 && !d_offset && !d_metres)) return rc;
  return launch_distance_call(ctx, map, vmin, dims, params, slice, d_d2, d_offset, d_metres);
}

int distance_host(loamx_ctx* ctx, loamx_occupancy_map* map, const int32_t* vmin, const uint32_t* dims, const loamx_distance_params* params, bool slice,
                  uint16_t* d2_out, int16_t* offset_out, float* metres_out) {
  API_ENTER(ctx);
  unsigned long long n = 0;
  int rc = distance_check(ctx, map, vmin, dims, params, slice, &n);
  if (rc != LOAMX_OK || n == 0 || (!d2_out && !offset_out && !metres_out)) return rc;
  const size_t axes = slice ? 2 : 3;
  const size_t o_off = align256(n * sizeof(uint16_t)), o_m = o_off + align256(n * axes * sizeof(int16_t));
  untimed(ctx);
  ENSURE(ctx, WS_OCC_OUT, o_m + n * sizeof(float));
  char* b = static_cast<char*>(ctx->ws[WS_OCC_OUT].p);
  rc = launch_distance_call(ctx, map, vmin, dims, params, slice, d2_out ? reinterpret_cast<uint16_t*>(b) : nullptr,
                            offset_out ? reinterpret_cast<int16_t*>(b + o_off) : nullptr, metres_out ? reinterpret_cast<float*>(b + o_m) : nullptr);
  if (rc != LOAMX_OK) return rc;
  if (d2_out) HIP_TRY(ctx, hipMemcpyAsync(d2_out, b, n * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream));
  if (offset_out) HIP_TRY(ctx, hipMemcpyAsync(offset_out, b + o_off, n * axes * sizeof(int16_t), hipMemcpyDeviceToHost, ctx->stream));
  if (metres_out) HIP_TRY(ctx, hipMemcpyAsync(metres_out, b + o_m, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LOAMX_OK;
}

}  // namespace

int loamx::occupancy_map_check(loamx_ctx* ctx, const loamx_occupancy_map* map) { return voxel_map_check(ctx, map, kKind); }

extern "C" {

void loamx_default_occupancy_params(loamx_occupancy_params* p) {
  if (!p) return;
  p->leaf = 0.2, p->min_range = 0.5, p->max_range = 80.0, p->end_margin = 0.2;
  p->clip_long = 1, p->min_hits = 1, p->occ_ratio = 0.0, p->min_passes = 1;
}

int loamx_occupancy_create(loamx_ctx* ctx, const loamx_occupancy_params* params, size_t max_voxels, loamx_occupancy_map** out) {
  API_ENTER(ctx);
  if (!params || !out) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  *out = nullptr;
  if (!isfinite(params->leaf) || !(params->leaf > 0.0)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "leaf must be finite and positive");
  if (bad_double(params->min_range) || bad_double(params->max_range) || bad_double(params->end_margin) || bad_double(params->occ_ratio))
    return fail(ctx, LOAMX_ERR_BAD_PARAM, "min_range, max_range, end_margin and occ_ratio must be finite and not negative");
  if (!(params->max_range >= params->min_range)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "max_range must be at least min_range");
  if (max_voxels == 0) return fail(ctx, LOAMX_ERR_BAD_PARAM, "max_voxels must be >= 1");
  if (params->max_range / params->leaf > 4096.0) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "max_range / leaf > 4096 not supported");
  if (max_voxels > kOccMaxVoxels) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "max_voxels > 2^30 not supported");
  loamx_occupancy_map* map = new loamx_occupancy_map;
  map->owner = ctx, map->device = ctx->device;
  map->params = *params;
  map->rule.leaf = params->leaf;
  map->rule.min_r2 = params->min_range * params->min_range, map->rule.max_r2 = params->max_range * params->max_range;
  map->rule.max_range = params->max_range, map->rule.end_margin = params->end_margin, map->rule.clip_long = params->clip_long ? 1u : 0u;
  map->state_rule.min_hits = params->min_hits, map->state_rule.min_passes = params->min_passes, map->state_rule.occ_ratio = params->occ_ratio;
  const uint32_t log2_cap = voxel_table_log2(2 * max_voxels);
  const size_t cap = (size_t)1 << log2_cap;
  const size_t o_keys = 0, o_counts = o_keys + align256(cap * sizeof(unsigned long long));
  const size_t o_words = o_counts + align256(cap * sizeof(unsigned long long));
  const size_t bytes = o_words + align256(kOccWords * sizeof(unsigned long long));
  hipError_t e = hipMalloc(&map->block, bytes);
  if (e != hipSuccess) {
    delete map;
    return fail(ctx, LOAMX_ERR_HIP, std::string("occupancy map storage: ") + hipGetErrorString(e));
  }
  char* b = static_cast<char*>(map->block);
  map->ones_bytes = o_counts, map->zeros_bytes = bytes - o_counts;
  map->t.keys = reinterpret_cast<unsigned long long*>(b + o_keys), map->t.counts = reinterpret_cast<unsigned long long*>(b + o_counts);
  map->t.words = reinterpret_cast<unsigned long long*>(b + o_words), map->t.log2_cap = log2_cap;
  int rc = voxel_map_clear(ctx, map);
  if (rc != LOAMX_OK) {
    (void)hipFree(map->block);
    delete map;
    return rc;
  }
  *out = map;
  return LOAMX_OK;
}

void loamx_occupancy_destroy(loamx_ctx* ctx, loamx_occupancy_map* map) {
  if (!map) return;
  voxel_map_destroy(ctx, map);
  if (map->dist_block) (void)hipFree(map->dist_block);  // (behind the stream's work: voxel_map_destroy has waited for it)
  delete map;
}

int loamx_occupancy_clear(loamx_ctx* ctx, loamx_occupancy_map* map) {
  API_ENTER(ctx);
  int rc = voxel_map_check(ctx, map, kKind);
  if (rc != LOAMX_OK) return rc;
  return voxel_map_clear(ctx, map);
}

int loamx_occupancy_crop(loamx_ctx* ctx, loamx_occupancy_map* map, const double* d_pose, const double lo[3], const double hi[3], uint32_t* d_counts_out) {
  CropTable t = {};
  if (map)
    t = {map->t.keys, map->t.counts, nullptr, nullptr, nullptr, nullptr, map->t.words + kOccWordVoxels, map->t.log2_cap, 1u,
         (uint32_t)1 << map->t.log2_cap};
  return voxel_map_crop(ctx, map, kKind, t, map ? map->rule.leaf : 0.0, d_pose, lo, hi, d_counts_out);
}

int loamx_occupancy_add_clouds_dev(loamx_ctx* ctx, loamx_occupancy_map* map, const double* d_points, size_t point_stride, const size_t* cloud_offsets,
                                   size_t n_clouds, const double* d_poses) {
  return voxel_map_add_dev(ctx, map, kKind, d_points, false, point_stride, cloud_offsets, n_clouds, d_poses);
}
int loamx_occupancy_add_clouds_dev_f32(loamx_ctx* ctx, loamx_occupancy_map* map, const float* d_points, size_t point_stride, const size_t* cloud_offsets,
                                       size_t n_clouds, const double* d_poses) {
  return voxel_map_add_dev(ctx, map, kKind, d_points, true, point_stride, cloud_offsets, n_clouds, d_poses);
}
int loamx_occupancy_add_cloud(loamx_ctx* ctx, loamx_occupancy_map* map, const double* points, size_t point_stride, size_t n_points, const double pose[7]) {
  return voxel_map_add_host(ctx, map, kKind, points, false, point_stride, n_points, pose);
}
int loamx_occupancy_add_cloud_f32(loamx_ctx* ctx, loamx_occupancy_map* map, const float* points, size_t point_stride, size_t n_points,
                                  const double pose[7]) {
  return voxel_map_add_host(ctx, map, kKind, points, true, point_stride, n_points, pose);
}

int loamx_occupancy_query_dev(loamx_ctx* ctx, const loamx_occupancy_map* map, const double* d_points, size_t point_stride, size_t n,
                              uint32_t* d_counts_out, uint8_t* d_state_out) {
  API_ENTER(ctx);
  int rc = query_check(ctx, map, d_points, point_stride, n);
  if (rc != LOAMX_OK || n == 0 || (!d_counts_out && !d_state_out)) return rc;
  untimed(ctx);
  launch_occupancy_query(map->t, map->rule.leaf, map->state_rule, d_points, (uint32_t)point_stride, n, d_counts_out, d_state_out, ctx->stream);
  CHECK_LAUNCH(ctx, "occupancy query kernel");
  return LOAMX_OK;
}

int loamx_occupancy_box_dev(loamx_ctx* ctx, const loamx_occupancy_map* map, const int32_t vmin[3], const uint32_t dims[3], uint32_t* d_counts_out,
                            uint8_t* d_state_out) {
  API_ENTER(ctx);
  unsigned long long n = 0;
  int rc = box_check(ctx, map, vmin, dims, true, &n);
  if (rc != LOAMX_OK || n == 0 || (!d_counts_out && !d_state_out)) return rc;
  return launch_box(ctx, map, vmin, dims, d_counts_out, d_state_out);
}

int loamx_occupancy_slice_dev(loamx_ctx* ctx, const loamx_occupancy_map* map, const int32_t vmin[3], const uint32_t dims[3], uint8_t* d_grid_out) {
  API_ENTER(ctx);
  unsigned long long n = 0;
  int rc = box_check(ctx, map, vmin, dims, false, &n);
  if (rc != LOAMX_OK || n == 0) return rc;
  if (!d_grid_out) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null d_grid_out");
  return launch_slice(ctx, map, vmin, dims, d_grid_out);
}

int loamx_occupancy_query(loamx_ctx* ctx, const loamx_occupancy_map* map, const double* points, size_t point_stride, size_t n, uint32_t* counts_out,
                          uint8_t* state_out) {
  API_ENTER(ctx);
  int rc = query_check(ctx, map, points, point_stride, n);
  if (rc != LOAMX_OK || n == 0 || (!counts_out && !state_out)) return rc;
  if (n > (~(size_t)0) / (point_stride * sizeof(double))) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "the points do not fit the address space");
  const size_t in_bytes = n * point_stride * sizeof(double);
  untimed(ctx);
  ENSURE(ctx, WS_OCC_IN, in_bytes);
  ENSURE(ctx, WS_OCC_OUT, align256(n * 2 * sizeof(uint32_t)) + n);
  HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[WS_OCC_IN].p, points, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  char* b = static_cast<char*>(ctx->ws[WS_OCC_OUT].p);
  launch_occupancy_query(map->t, map->rule.leaf, map->state_rule, wsp<double>(ctx, WS_OCC_IN), (uint32_t)point_stride, n, reinterpret_cast<uint32_t*>(b),
                         reinterpret_cast<uint8_t*>(b + align256(n * 2 * sizeof(uint32_t))), ctx->stream);
  rc = check_launch(ctx, "occupancy query kernel");
  if (rc != LOAMX_OK) {
    (void)hipStreamSynchronize(ctx->stream);  // (the upload must not outlive the caller's array)
    return rc;
  }
  return read_out(ctx, n, counts_out, state_out);
}

int loamx_occupancy_box(loamx_ctx* ctx, const loamx_occupancy_map* map, const int32_t vmin[3], const uint32_t dims[3], uint32_t* counts_out,
                        uint8_t* state_out) {
  API_ENTER(ctx);
  unsigned long long n = 0;
  int rc = box_check(ctx, map, vmin, dims, true, &n);
  if (rc != LOAMX_OK || n == 0 || (!counts_out && !state_out)) return rc;
  untimed(ctx);
  ENSURE(ctx, WS_OCC_OUT, align256(n * 2 * sizeof(uint32_t)) + n);
  char* b = static_cast<char*>(ctx->ws[WS_OCC_OUT].p);
  rc = launch_box(ctx, map, vmin, dims, reinterpret_cast<uint32_t*>(b), reinterpret_cast<uint8_t*>(b + align256(n * 2 * sizeof(uint32_t))));
  if (rc != LOAMX_OK) return rc;
  return read_out(ctx, n, counts_out, state_out);
}

int loamx_occupancy_slice(loamx_ctx* ctx, const loamx_occupancy_map* map, const int32_t vmin[3], const uint32_t dims[3], uint8_t* grid_out) {
  API_ENTER(ctx);
  unsigned long long n = 0;
  int rc = box_check(ctx, map, vmin, dims, false, &n);
  if (rc != LOAMX_OK || n == 0) return rc;
  if (!grid_out) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null grid_out");
  untimed(ctx);
  ENSURE(ctx, WS_OCC_OUT, n);
  rc = launch_slice(ctx, map, vmin, dims, wsp<uint8_t>(ctx, WS_OCC_OUT));
  if (rc != LOAMX_OK) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(grid_out, ctx->ws[WS_OCC_OUT].p, n, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LOAMX_OK;
}

void loamx_default_distance_params(loamx_distance_params* p) {
  if (!p) return;
  p->max_dist_voxels = 10, p->unknown_is_obstacle = 0;
}

int loamx_occupancy_distance_box(loamx_ctx* ctx, loamx_occupancy_map* map, const int32_t vmin[3], const uint32_t dims[3],
                                 const loamx_distance_params* params, uint16_t* d_d2_out, int16_t* d_offset_out, float* d_metres_out) {
  return distance_dev(ctx, map, vmin, dims, params, false, d_d2_out, d_offset_out, d_metres_out);
}
int loamx_occupancy_distance_slice(loamx_ctx* ctx, loamx_occupancy_map* map, const int32_t vmin[3], const uint32_t dims[3],
                                   const loamx_distance_params* params, uint16_t* d_d2_out, int16_t* d_offset_out, float* d_metres_out) {
  return distance_dev(ctx, map, vmin, dims, params, true, d_d2_out, d_offset_out, d_metres_out);
}
int loamx_occupancy_distance_box_host(loamx_ctx* ctx, loamx_occupancy_map* map, const int32_t vmin[3], const uint32_t dims[3],
                                      const loamx_distance_params* params, uint16_t* d2_out, int16_t* offset_out, float* metres_out) {
  return distance_host(ctx, map, vmin, dims, params, false, d2_out, offset_out, metres_out);
}
int loamx_occupancy_distance_slice_host(loamx_ctx* ctx, loamx_occupancy_map* map, const int32_t vmin[3], const uint32_t dims[3],
                                        const loamx_distance_params* params, uint16_t* d2_out, int16_t* offset_out, float* metres_out) {
  return distance_host(ctx, map, vmin, dims, params, true, d2_out, offset_out, metres_out);
}

int loamx_occupancy_stats_read(loamx_ctx* ctx, const loamx_occupancy_map* map, loamx_occupancy_stats* out) {
  API_ENTER(ctx);
  int rc = voxel_map_check(ctx, map, kKind);
  if (rc != LOAMX_OK) return rc;
  if (!out) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  unsigned long long words[kOccWords];
  untimed(ctx);
  HIP_TRY(ctx, hipMemcpyAsync(words, map->t.words, sizeof(words), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  out->rays_offered = map->offered, out->rays_hit = words[kOccWordHit], out->invalid = words[kOccWordInvalid];
  out->range_short = words[kOccWordShort], out->range_long = words[kOccWordLong], out->outside = words[kOccWordOutside];
  out->visits = words[kOccWordVisits], out->voxels = words[kOccWordVoxels], out->overflow = words[kOccWordOverflow];
  return LOAMX_OK;
}

int loamx_occupancy_claims_read(loamx_ctx* ctx, const loamx_occupancy_map* map, uint64_t* claims) {
  return voxel_map_read_word(ctx, map, kKind, map ? map->t.words + kOccWordClaims : nullptr, claims);
}

}  // extern "C"
