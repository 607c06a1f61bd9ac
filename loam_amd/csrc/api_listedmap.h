// api_listedmap.h — the host side of a listed voxel table (ListedTable of loamx_internal.h), written once for the cloud map
// (api_cloudmap.hip) and the surfel map (api_surfel.hip): the two handles with their one device block (table, voxel list, counters,
// the scratch of a round of launches), create, the add loop, clear, crop, destroy, the stats and claims read-outs and the read-back of
// a host emit. A map adds its parameters, its emit and whatever only it can do. api_localize.hip reads the surfel map's table and rule.
#pragma once
#include "api_voxelmap.h"

namespace loamx {

struct ListedMapBase : VoxelMapBase {  // ones: keys + first; zeros: payload, count, counters and lengths
  CloudRule rule = {};
  ListedTable t = {};
  uint32_t* d_slot = nullptr;   // scratch of a round of an add: [kCloudChunkPoints]
  uint8_t* d_keep = nullptr;    // [max(kCloudChunkPoints, max_voxels)] (add and emit)
  uint32_t* d_tiles = nullptr;  // the compaction's tiles for as many
};

struct ListedMapKind : VoxelMapKind {
  uint32_t slot_words;                 // 64-bit words of a slot's payload
  ListedAccumulate* accumulate;
  uint32_t no_combine_flag;            // (loamx_ctx::reg_flags) one claim per point
  int k_combined, k_plain, k_list;     // the timing rows of an add's accumulate (either form) and list launches; -1: the add is untimed
};

}  // namespace loamx

struct loamx_cloud_map : loamx::ListedMapBase {
  loamx_cloud_map_params params = {};
};
struct loamx_surfel_map : loamx::ListedMapBase {
  loamx_surfel_map_params params = {};
};

namespace loamx {

constexpr size_t kListedMaxVoxels = (size_t)1 << 30;

// VoxelMapKind::add_locked of both maps: the clouds of the call chunk by chunk, their points in rounds of kCloudChunkPoints;
// `offered` is the running index of the call's first point
inline int listed_map_add_locked(loamx_ctx* ctx, VoxelMapBase* base, const VoxelMapKind& base_kind, const void* d_points, bool f32, size_t stride,
                                 const size_t* offsets, size_t n_clouds, const double* d_poses) {
  ListedMapBase* map = static_cast<ListedMapBase*>(base);
  const ListedMapKind& kind = static_cast<const ListedMapKind&>(base_kind);
  const bool combine = !(ctx->reg_flags & kind.no_combine_flag);
  const double point_bytes = f32 ? 12.0 : 24.0;
  untimed(ctx);
  for (CloudChunks ch(offsets, n_clouds); ch.next();) {
    for (unsigned long long p0 = ch.offs.off[0]; p0 < ch.offs.off[ch.nc]; p0 += kCloudChunkPoints) {
      const uint32_t n = (uint32_t)(ch.offs.off[ch.nc] - p0 < kCloudChunkPoints ? ch.offs.off[ch.nc] - p0 : kCloudChunkPoints);
      const uint32_t g0 = (uint32_t)(map->offered + (p0 - offsets[0]));
      {
        TimedScope timed(ctx, combine ? kind.k_combined : kind.k_plain, point_bytes * n, true);
        kind.accumulate(d_points, f32, (uint32_t)stride, ch.offs, ch.nc, p0, n, g0, d_poses ? d_poses + ch.c0 * 7 : nullptr, map->rule, map->t, combine,
                        map->d_slot, ctx->stream);
      }
      {
        TimedScope timed(ctx, kind.k_list, 5.0 * n, true);
        launch_listed_list(map->t, map->d_slot, n, g0, map->d_keep, map->d_tiles, ctx->stream);
      }
      CHECK_LAUNCH(ctx, (std::string(kind.name) + " add kernels").c_str());
    }
  }
  map->offered += offsets[n_clouds] - offsets[0];
  return LOAMX_OK;
}

// the checks, the one device block and its carve, and an empty map. Params: leaf, min_range, max_range.
template <typename Map, typename Params>
int listed_map_create(loamx_ctx* ctx, const ListedMapKind& kind, const Params* params, size_t max_voxels, Map** out) {
  API_ENTER(ctx);
  if (!params || !out) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  *out = nullptr;
  if (!isfinite(params->leaf) || !(params->leaf > 0.0)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "leaf must be finite and positive");
  if (!isfinite(params->min_range) || params->min_range < 0.0) return fail(ctx, LOAMX_ERR_BAD_PARAM, "min_range must be finite and not negative");
  if (!(params->max_range >= params->min_range)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "max_range must be at least min_range");
  if (max_voxels == 0) return fail(ctx, LOAMX_ERR_BAD_PARAM, "max_voxels must be >= 1");
  if (max_voxels > kListedMaxVoxels) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "max_voxels > 2^30 not supported");
  Map* map = new Map;
  map->owner = ctx, map->device = ctx->device;
  map->params = *params;
  map->rule.leaf = params->leaf;
  map->rule.min_r2 = params->min_range * params->min_range, map->rule.max_r2 = params->max_range * params->max_range;
  const uint32_t log2_cap = voxel_table_log2(2 * max_voxels);
  const size_t cap = (size_t)1 << log2_cap, scratch = max_voxels > kCloudChunkPoints ? max_voxels : kCloudChunkPoints;
  const size_t o_keys = 0, o_first = o_keys + align256(cap * sizeof(unsigned long long));
  const size_t o_payload = o_first + align256(cap * sizeof(uint32_t)), o_count = o_payload + align256(cap * kind.slot_words * sizeof(unsigned long long));
  const size_t o_words = o_count + align256(cap * sizeof(uint32_t)), o_lens = o_words + align256(kCloudWords * sizeof(unsigned long long));
  const size_t o_list = o_lens + align256(kCloudLens * sizeof(uint32_t)), o_slot = o_list + align256(max_voxels * sizeof(uint32_t));
  const size_t o_keep = o_slot + align256((size_t)kCloudChunkPoints * sizeof(uint32_t)), o_tiles = o_keep + align256(scratch);
  const size_t bytes = o_tiles + align256(map_compact_ws_bytes(scratch));
  hipError_t e = hipMalloc(&map->block, bytes);
  if (e != hipSuccess) {
    delete map;
    return fail(ctx, LOAMX_ERR_HIP, std::string(kind.name) + " storage: " + hipGetErrorString(e));
  }
  char* b = static_cast<char*>(map->block);
  map->ones_bytes = o_payload, map->zeros_bytes = o_list - o_payload;
  map->t.keys = reinterpret_cast<unsigned long long*>(b + o_keys), map->t.first = reinterpret_cast<uint32_t*>(b + o_first);
  map->t.payload = reinterpret_cast<unsigned long long*>(b + o_payload), map->t.count = reinterpret_cast<uint32_t*>(b + o_count);
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

template <typename Map>
void listed_map_destroy(loamx_ctx* ctx, Map* map) {
  if (!map) return;
  voxel_map_destroy(ctx, map);
  delete map;
}

inline int listed_map_clear(loamx_ctx* ctx, ListedMapBase* map, const ListedMapKind& kind) {
  API_ENTER(ctx);
  int rc = voxel_map_check(ctx, map, kind);
  if (rc != LOAMX_OK) return rc;
  return voxel_map_clear(ctx, map);
}

// a listed table as the crop sees it
inline CropTable crop_table(const ListedTable& t, uint32_t payload_words) {
  return {t.keys, t.payload, t.first, t.count, t.list, t.lens + kCloudLenListed, nullptr, t.log2_cap, payload_words, t.max_voxels};
}

inline int listed_map_crop(loamx_ctx* ctx, ListedMapBase* map, const ListedMapKind& kind, const double* d_pose, const double lo[3], const double hi[3],
                           uint32_t* d_counts_out) {
  return voxel_map_crop(ctx, map, kind, map ? crop_table(map->t, kind.slot_words) : CropTable{}, map ? map->rule.leaf : 0.0, d_pose, lo, hi, d_counts_out);
}

// the two public stats structs are the same seven 64-bit fields under two names
template <typename Stats>
int listed_map_stats_read(loamx_ctx* ctx, const ListedMapBase* map, const ListedMapKind& kind, Stats* out) {
  static_assert(sizeof(Stats) == 7 * sizeof(uint64_t), "voxels, points_offered, points_used, invalid, range, outside, overflow");
  API_ENTER(ctx);
  int rc = voxel_map_check(ctx, map, kind);
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

inline int listed_map_claims_read(loamx_ctx* ctx, const ListedMapBase* map, const ListedMapKind& kind, uint64_t* claims) {
  return voxel_map_read_word(ctx, map, kind, map ? map->t.words + kCloudWordClaims : nullptr, claims);
}

// The read-back of a host emit, behind its kernels: the number of qualifying voxels n from d_n (synchronises), then min(n, capacity)
// records of each array with a destination, then *n_out = n.
struct EmitCopy {
  void* dst;  // may be nullptr: not asked for
  const void* d_src;
  size_t record_bytes;
};
inline int listed_emit_read(loamx_ctx* ctx, const void* d_n, size_t capacity, const EmitCopy* copies, int n_copies, size_t* n_out) {
  untimed(ctx);
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_pinned, d_n, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  const size_t n = ctx->h_pinned[0], m = n < capacity ? n : capacity;
  if (m) {
    for (int c = 0; c < n_copies; c++)
      if (copies[c].dst) HIP_TRY(ctx, hipMemcpyAsync(copies[c].dst, copies[c].d_src, m * copies[c].record_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  *n_out = n;
  return LOAMX_OK;
}

}  // namespace loamx
