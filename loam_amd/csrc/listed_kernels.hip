// listed_kernels.hip — the voxel list of a listed voxel table (ListedTable of loamx_internal.h), for the cloud map and the surfel map
// alike: nothing here touches a slot's payload. The stable compaction is the one of map_kernels.hip (map_compact.h).
//
// An add is five launches per chunk of points: the map's accumulate (listed_accumulate.h), then launch_listed_list: the flags of the
// points that opened a voxel, the two launches of the compaction's tile offsets, the append of the flagged points' slots to the
// list, and one thread that adds the chunk's new voxels to the list's length. An emit is launch_listed_emit_flags (flags over the
// list, the tile offsets) and the map's own scatter. No launch waits for another workgroup, and every loop has a bound that does
// not depend on the data.
#include "listed_accumulate.h"
#include "map_compact.h"

namespace loamx {
namespace {

// behind the accumulate (plain loads are fine across the kernel boundary): point g opened its voxel iff the voxel's `first` is g. A
// voxel that existed before the chunk has a smaller `first`, so this is also "the voxel did not exist before the call".
__global__ __launch_bounds__(kListedThreads) void listed_new_flags_kernel(const uint32_t* __restrict__ first, const uint32_t* __restrict__ slot,
                                                                          uint32_t n, uint32_t g0, uint8_t* __restrict__ keep) {
  const uint32_t i = blockIdx.x * kListedThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = slot[i];
  keep[i] = s != kMapNoSlot && first[s] == g0 + i;
}

// the flagged points' slots behind the list's present end, in input order; what does not fit is counted, never written
__global__ __launch_bounds__(kListedThreads) void listed_append_kernel(const uint8_t* __restrict__ keep, const uint32_t* __restrict__ slot, uint32_t n,
                                                                       const uint32_t* __restrict__ tiles, ListedTable t) {
  __shared__ uint32_t s_wave[4];
  const uint32_t i = blockIdx.x * kListedThreads + threadIdx.x;
  const bool flag = i < n && keep[i] != 0;
  uint32_t total;
  const uint32_t rank = block_rank(flag, s_wave, total);
  if (!flag) return;
  const unsigned long long dst = (unsigned long long)t.lens[kCloudLenListed] + tiles[blockIdx.x] + rank;
  if (dst < t.max_voxels) t.list[dst] = slot[i];
  else atomicAdd(t.words + kCloudWordOverflow, 1ull);
}

// one thread, behind the append: the list has grown by the chunk's new voxels (those that fitted)
__global__ void listed_commit_kernel(ListedTable t) {
  const unsigned long long len = (unsigned long long)t.lens[kCloudLenListed] + t.lens[kCloudLenPending];
  t.lens[kCloudLenListed] = len < t.max_voxels ? (uint32_t)len : t.max_voxels;
}

// one thread per list entry up to the list's capacity (its length is known on the device only)
__global__ __launch_bounds__(kListedThreads) void listed_emit_flags_kernel(ListedTable t, uint32_t min_points, uint8_t* __restrict__ keep) {
  const uint32_t j = blockIdx.x * kListedThreads + threadIdx.x;
  if (j >= t.max_voxels) return;
  keep[j] = j < t.lens[kCloudLenListed] && t.count[t.list[j]] >= min_points;
}

}  // namespace

void launch_listed_list(const ListedTable& t, const uint32_t* d_slot, uint32_t n, uint32_t g0, uint8_t* d_keep, uint32_t* d_tiles, hipStream_t s) {
  launch_kernel(listed_new_flags_kernel, listed_tiles(n), dim3(kListedThreads), 0, s, (const uint32_t*)t.first, d_slot, n, g0, d_keep);
  launch_tile_offsets(d_keep, n, d_tiles, t.lens + kCloudLenPending, s);
  launch_kernel(listed_append_kernel, listed_tiles(n), dim3(kListedThreads), 0, s, (const uint8_t*)d_keep, d_slot, n, (const uint32_t*)d_tiles, t);
  launch_kernel(listed_commit_kernel, dim3(1), dim3(1), 0, s, t);
}

void launch_listed_emit_flags(const ListedTable& t, uint32_t min_points, uint8_t* d_keep, uint32_t* d_tiles, uint32_t* d_n_out, hipStream_t s) {
  launch_kernel(listed_emit_flags_kernel, listed_tiles(t.max_voxels), dim3(kListedThreads), 0, s, t, min_points, d_keep);
  launch_tile_offsets(d_keep, t.max_voxels, d_tiles, d_n_out, s);
}

}  // namespace loamx
