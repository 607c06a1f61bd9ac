// api_voxelmap.h — the host side that the handles of the three voxel maps share (the cloud map and the surfel map through
// api_listedmap.h, the occupancy map in api_occupancy.hip): the head of the handle, the checks, clear, crop and destroy, and the two
// forms of an add around the map's own add_locked. Each map names itself in a VoxelMapKind, so every error text reads as that map's.
#pragma once
#include "api_host.h"

namespace loamx {

// a map handle starts with this (ListedMapBase and loamx_occupancy_map derive from it)
struct VoxelMapBase {
  loamx_ctx* owner = nullptr;  // the context it was created on: its mutex and stream order every use
  int device = 0;
  void* block = nullptr;       // the one device allocation: table, counters and whatever else the map keeps
  size_t ones_bytes = 0;       // at the block's start (the keys first): 0xFF bytes in an empty map
  size_t zeros_bytes = 0;      // behind them: zero bytes in an empty map
  uint64_t offered = 0;        // points or rays offered since the last clear (the cloud map's running index of the next call)
  void* crop_block = nullptr;  // the scratch of a crop (crop_kernels.hip), allocated at the handle's first crop, freed at destroy
};

struct VoxelMapKind {
  const char *name, *a_name, *items;  // "cloud map", "a cloud map", "points"
  uint64_t max_offered;               // items between two clears
  int ws_in, ws_pose;                 // the workspace the host form of an add uploads to
  // the map's launches for checked arguments (kind: this record); the caller holds ctx->mu and has selected the device
  int (*add_locked)(loamx_ctx* ctx, VoxelMapBase* map, const VoxelMapKind& kind, const void* d_points, bool f32, size_t stride, const size_t* offsets, size_t n_clouds,
                    const double* d_poses);
};

inline int voxel_map_check(loamx_ctx* ctx, const VoxelMapBase* map, const VoxelMapKind& kind) {
  if (!map) return fail(ctx, LOAMX_ERR_BAD_PARAM, std::string("null ") + kind.name);
  if (map->owner != ctx) return fail(ctx, LOAMX_ERR_BAD_PARAM, std::string("the ") + kind.name + " was created on another context");
  return LOAMX_OK;
}

inline int voxel_map_clear(loamx_ctx* ctx, VoxelMapBase* map) {
  untimed(ctx);
  HIP_TRY(ctx, hipMemsetAsync(map->block, 0xFF, map->ones_bytes, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(static_cast<char*>(map->block) + map->ones_bytes, 0, map->zeros_bytes, ctx->stream));
  map->offered = 0;
  return LOAMX_OK;
}

// frees the block, behind the kernels still working on the map when there is a context; the caller deletes the handle
inline void voxel_map_destroy(loamx_ctx* ctx, VoxelMapBase* map) {
  std::unique_lock<std::mutex> guard;
  if (ctx) {
    guard = std::unique_lock<std::mutex>(ctx->mu);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  if (map->block) (void)hipFree(map->block);
  if (map->crop_block) (void)hipFree(map->crop_block);
}

// The map window (loamx.h, "map window") of any of the three maps: `t` is the map's table as the crop sees it. The checks and their
// texts are those of loamx_target_index_crop; a refused call changes nothing. The handle's first crop allocates the scratch (and
// may wait on the allocator), every later one only enqueues. The counters, `offered` and the overflow word are not touched.
inline int voxel_map_crop(loamx_ctx* ctx, VoxelMapBase* map, const VoxelMapKind& kind, const CropTable& t, double leaf, const double* d_pose,
                          const double* lo, const double* hi, uint32_t* d_counts_out) {
  API_ENTER(ctx);
  int rc = voxel_map_check(ctx, map, kind);
  if (rc != LOAMX_OK) return rc;
  if (!lo || !hi) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  for (int c = 0; c < 3; c++)
    if (!(lo[c] <= hi[c])) return fail(ctx, LOAMX_ERR_BAD_PARAM, "crop box: lo <= hi on every axis (and no NaN)");
  if (!map->crop_block) {
    hipError_t e = hipMalloc(&map->crop_block, crop_scratch_bytes(t));
    if (e != hipSuccess) {
      map->crop_block = nullptr;
      return fail(ctx, LOAMX_ERR_HIP, std::string(kind.name) + " crop scratch: " + hipGetErrorString(e));
    }
  }
  untimed(ctx);
  launch_voxel_crop(t, crop_scratch_carve(map->crop_block, t), leaf, d_pose, lo, hi, d_counts_out, ctx->stream);
  CHECK_LAUNCH(ctx, "map crop kernels");
  return LOAMX_OK;
}

// the argument checks the device and the host forms of an add share; *total: the items of the call
inline int voxel_map_add_check(loamx_ctx* ctx, const VoxelMapBase* map, const VoxelMapKind& kind, const void* points, size_t stride,
                               const size_t* offsets, size_t n_clouds, size_t* total) {
  int rc = voxel_map_check(ctx, map, kind);
  if (rc != LOAMX_OK) return rc;
  *total = 0;
  if (stride < 3) return fail(ctx, LOAMX_ERR_BAD_PARAM, "point_stride must be >= 3");
  if (stride > 0xFFFFFFFFull) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "point_stride does not fit 32 bits");
  if (n_clouds == 0) return LOAMX_OK;
  if (!offsets) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null cloud_offsets");
  for (size_t c = 0; c < n_clouds; c++)
    if (offsets[c + 1] < offsets[c]) return fail(ctx, LOAMX_ERR_BAD_PARAM, "cloud_offsets must ascend");
  *total = offsets[n_clouds] - offsets[0];
  if (*total && !points) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null points");
  if (*total > kind.max_offered || map->offered + *total > kind.max_offered)
    return fail(ctx, LOAMX_ERR_UNSUPPORTED, std::string(kind.a_name) + " takes at most 2^32 - 2 " + kind.items + " between two clears");
  return LOAMX_OK;
}

inline int voxel_map_add_dev(loamx_ctx* ctx, VoxelMapBase* map, const VoxelMapKind& kind, const void* d_points, bool f32, size_t stride,
                             const size_t* offsets, size_t n_clouds, const double* d_poses) {
  API_ENTER(ctx);
  size_t total = 0;
  int rc = voxel_map_add_check(ctx, map, kind, d_points, stride, offsets, n_clouds, &total);
  if (rc != LOAMX_OK || total == 0) return rc;
  return kind.add_locked(ctx, map, kind, d_points, f32, stride, offsets, n_clouds, d_poses);
}

// one cloud in host memory: upload, the device path, synchronise
inline int voxel_map_add_host(loamx_ctx* ctx, VoxelMapBase* map, const VoxelMapKind& kind, const void* points, bool f32, size_t stride, size_t n,
                              const double* pose) {
  API_ENTER(ctx);
  const size_t offsets[2] = {0, n};
  size_t total = 0;
  int rc = voxel_map_add_check(ctx, map, kind, points, stride, offsets, 1, &total);
  if (rc != LOAMX_OK || total == 0) return rc;
  if (n > (~(size_t)0) / (stride * sizeof(double))) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "the cloud does not fit the address space");
  const size_t in_bytes = n * stride * (f32 ? sizeof(float) : sizeof(double));
  untimed(ctx);
  ENSURE(ctx, kind.ws_in, in_bytes);
  ENSURE(ctx, kind.ws_pose, 7 * sizeof(double));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[kind.ws_in].p, points, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (pose) HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[kind.ws_pose].p, pose, 7 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  rc = kind.add_locked(ctx, map, kind, ctx->ws[kind.ws_in].p, f32, stride, offsets, 1, pose ? wsp<double>(ctx, kind.ws_pose) : nullptr);
  if (rc != LOAMX_OK) {
    (void)hipStreamSynchronize(ctx->stream);  // (the upload must not outlive the caller's array)
    return rc;
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LOAMX_OK;
}

// one counter word of the map to the host (synchronises); d_word is not looked at before the map has passed its check
inline int voxel_map_read_word(loamx_ctx* ctx, const VoxelMapBase* map, const VoxelMapKind& kind, const unsigned long long* d_word, uint64_t* out) {
  API_ENTER(ctx);
  int rc = voxel_map_check(ctx, map, kind);
  if (rc != LOAMX_OK) return rc;
  if (!out) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  unsigned long long word = 0;
  untimed(ctx);
  HIP_TRY(ctx, hipMemcpyAsync(&word, d_word, sizeof(word), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *out = word;
  return LOAMX_OK;
}

}  // namespace loamx
