// surfel_slot.h — the record of one slot of a surfel table, read by plain loads behind a kernel boundary from the last add. Device
// only; shared by the read-outs of surfel_kernels.hip and the plain form of localize_kernels.hip.
#pragma once
#include "loamx_internal.h"
#include "surfel_math.h"

namespace loamx {

__device__ __forceinline__ loamx_surfel surfel_of_slot(const ListedTable& t, uint32_t s, uint32_t count, double leaf) {
  const unsigned long long* w = t.payload + (size_t)s * kSurfelSlotWords;
  uint64_t sum[3], S[6];
  int64_t W[3];
#pragma unroll
  for (int a = 0; a < 3; a++) sum[a] = w[a], W[a] = (int64_t)w[9 + a];
#pragma unroll
  for (int a = 0; a < 6; a++) S[a] = w[3 + a];
  return surfel_finish(t.keys[s], sum, S, W, count, t.first[s], leaf);
}

}  // namespace loamx
