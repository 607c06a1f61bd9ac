// map_compact.h — the stable compaction of map_kernels.hip for the kernels of other units (cloudmap_kernels.hip): the rank of a
// flagged thread inside its tile, and the two launches that turn per-point flags into the tiles' first output positions. A unit
// writes its own scatter kernel around block_rank: flagged thread -> tiles[blockIdx.x] + rank. Device code only.
#pragma once
#include "loamx_internal.h"

namespace loamx {

static_assert(kMapTile == 256, "block_rank and tile_scan_kernel are written for four wavefronts");

// rank of this thread among the flagged threads of its workgroup of kMapTile threads (in thread order) and their number;
// s_wave: four words of LDS. Every thread of the workgroup must call it.
__device__ __forceinline__ uint32_t block_rank(bool flag, uint32_t* s_wave, uint32_t& total) {
  const unsigned long long b = __ballot(flag);
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  if (lane == 0) s_wave[w] = (uint32_t)__popcll(b);
  __syncthreads();
  uint32_t before = 0;
  total = 0;
  for (uint32_t j = 0; j < 4; j++) {
    const uint32_t c = s_wave[j];
    before += j < w ? c : 0u;
    total += c;
  }
  return before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
}

// tile_count_kernel (skipped for n == 0) + tile_scan_kernel: d_tiles[t] = flagged points in front of tile t, *d_total = their
// number (written also for n == 0). d_tiles: map_compact_ws_bytes(n).
void launch_tile_offsets(const uint8_t* d_keep, uint32_t n, uint32_t* d_tiles, uint32_t* d_total, hipStream_t s);

}  // namespace loamx
