// xcd_map.h — workgroup -> (pair, chunk) placement of the kernels that are launched per pair and chunk. Host + device:
// tests/hostcheck_live compiles this file with g++ and walks every workgroup of small grids.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LOAMX_XCD_HD __host__ __device__ __forceinline__
#else
#define LOAMX_XCD_HD inline
#endif

namespace loamx {

// Workgroup -> (pair, chunk) mapping: workgroups are dealt round-robin over the 8 XCDs, so all
// chunks of one pair are given ids with the same id % 8 and share one XCD's L2 (the pair's target
// index + points are ~0.5 MB). With fewer than 8 pairs (single registrations, scan-to-map) that would
// leave XCDs idle, so the chunks are spread over all of them instead. Placement only affects speed,
// never results. (Grids are sized ceil(n_pairs / 8) * 8 * blocks_per_pair for both mappings.)
LOAMX_XCD_HD bool xcd_pair_map(uint32_t block, uint32_t blocks_per_pair, size_t n_pairs, size_t& pair, uint32_t& chunk) {
  if (n_pairs < 8) {
    pair = block / blocks_per_pair;
    chunk = block % blocks_per_pair;
  } else {
    const uint32_t xcd = block & 7u, slot = block >> 3;
    pair = (size_t)xcd + 8u * (size_t)(slot / blocks_per_pair);
    chunk = slot % blocks_per_pair;
  }
  return pair < n_pairs;
}

// The same deal over a list of the pairs that still run (live[0 .. n_live), any order): the arithmetic of xcd_pair_map gives
// an index into the list instead of a pair, so consecutive entries go to consecutive XCD lanes (the lanes' pair counts differ
// by one at most, however the finished pairs are spread over the batch) and all chunks of a pair still share one lane. For
// batches of at least 8 pairs, in the grids of xcd_pair_map; a workgroup past the list has nothing to do.
LOAMX_XCD_HD bool xcd_live_map(uint32_t block, uint32_t blocks_per_pair, size_t n_pairs, uint32_t n_live, const uint32_t* live, size_t& pair,
                               uint32_t& chunk) {
  const uint32_t xcd = block & 7u, slot = block >> 3;
  const size_t idx = (size_t)xcd + 8u * (size_t)(slot / blocks_per_pair);
  chunk = slot % blocks_per_pair;
  if (idx >= n_live || idx >= n_pairs) return false;
  pair = live[idx];
  return pair < n_pairs;
}

}  // namespace loamx
