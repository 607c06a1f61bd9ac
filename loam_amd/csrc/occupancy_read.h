// occupancy_read.h — what the read-outs of the occupancy map share (occupancy_kernels.hip: query, box, slice; distance_kernels.hip:
// the obstacle mask): the count word of a voxel and the key of a voxel of a box. Device only; plain loads, so only behind a kernel
// boundary from the last claim (voxel_table.h).
#pragma once
#include "loamx_internal.h"
#include "voxel_table.h"

namespace loamx {

// the count word of a voxel, 0 without a slot
__device__ __forceinline__ unsigned long long occ_lookup(const OccTable& t, uint64_t key) {
  const uint32_t s = voxel_find(t.keys, t.log2_cap, key);
  return s != kMapNoSlot ? t.counts[s] : 0ull;
}

// the key of voxel (vx, vy, vz); false outside |v| < 2^20
__device__ __forceinline__ bool occ_voxel_key(long long vx, long long vy, long long vz, uint64_t& key) {
  const bool ok = vx > -1048576ll && vx < 1048576ll && vy > -1048576ll && vy < 1048576ll && vz > -1048576ll && vz < 1048576ll;
  key = ok ? voxel_pack((uint64_t)(vx + 1048576ll), (uint64_t)(vy + 1048576ll), (uint64_t)(vz + 1048576ll)) : 0ull;
  return ok;
}

// the key of voxel vmin + (x, y, z); false outside |v| < 2^20
__device__ __forceinline__ bool occ_box_key(const OccBox& box, uint32_t x, uint32_t y, uint32_t z, uint64_t& key) {
  return occ_voxel_key((long long)box.vmin[0] + x, (long long)box.vmin[1] + y, (long long)box.vmin[2] + z, key);
}

}  // namespace loamx
