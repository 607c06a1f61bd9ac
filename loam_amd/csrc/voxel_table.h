// voxel_table.h — what the kernels of the three open-addressed voxel tables share (the occupancy table of the filtered insert in
// map_kernels.hip, the cloud map in cloudmap_kernels.hip, the occupancy map in occupancy_kernels.hip): the claim of a slot, the
// lookup behind a kernel boundary, the run heads of the combining forms, and the cloud and point of a row of a call's array.
// Device only. What a map does with a slot or with a run stays in its own kernel.
#pragma once
#include "loamx_internal.h"
#include "map_math.h"

namespace loamx {

/* THE RULE OF THE TABLE. A table is 2^log2_cap key slots that start as kVoxelEmpty; a key never leaves its slot before the
 * whole table is cleared. A thread that wants the slot of `key` probes linearly from voxel_hash(key), and
 *   - EVERY probe is a 64-bit atomicCAS(empty -> key) on the key slot, and the value it returns alone decides: empty (the slot
 *     is now this key's: `opened`), the key itself (another thread was first) or another key (next slot);
 *   - NO key slot is read by a plain load in a launch that claims: the L2s of the eight XCDs are not coherent with each other,
 *     and a line one of them holds may be older than a claim made through another;
 *   - atomics are performed at the memory side, which is why the value a CAS returns can be trusted where a load cannot;
 *   - the probe ends after `capacity` slots at the latest (never reached while the table is at most half full) and the caller
 *     counts what it stood for as given up: returns kMapNoSlot, has written nothing.
 * Which slot a key ends up in depends on which thread came first; nothing may read that. The mask is formed in 64 bits: 1u << 32
 * is not defined. */
__device__ __forceinline__ uint32_t voxel_claim(unsigned long long* keys, uint32_t log2_cap, uint64_t key, bool& opened) {
  const uint32_t mask = (uint32_t)((1ull << log2_cap) - 1ull);
  uint32_t s = voxel_hash(key, log2_cap), slot = kMapNoSlot;
  opened = false;
  for (uint32_t probe = 0; probe <= mask; probe++) {
    const unsigned long long old = atomicCAS(keys + s, (unsigned long long)kVoxelEmpty, (unsigned long long)key);
    if (old == kVoxelEmpty || old == key) {
      opened = old == kVoxelEmpty;
      slot = s;
      break;
    }
    s = (s + 1u) & mask;
  }
  return slot;
}

// The slot of `key`, kMapNoSlot without one: the same slot sequence by plain loads, so only BEHIND a kernel boundary from the
// last claim (a read-out on the same stream).
__device__ __forceinline__ uint32_t voxel_find(const unsigned long long* __restrict__ keys, uint32_t log2_cap, uint64_t key) {
  const uint32_t mask = (uint32_t)((1ull << log2_cap) - 1ull);
  uint32_t s = voxel_hash(key, log2_cap);
  for (uint32_t probe = 0; probe <= mask; probe++) {
    const unsigned long long k = keys[s];
    if (k == key) return s;
    if (k == kVoxelEmpty) return kMapNoSlot;
    s = (s + 1u) & mask;
  }
  return kMapNoSlot;
}

// Run combining: lanes that are `on` and hold the same key in ADJACENT lanes form a run (A B A is three runs); true in the
// first lane of every run. m_on = __ballot(on). Every lane of the wavefront calls it (the key of the lane before comes by shuffle).
__device__ __forceinline__ bool run_head(bool on, uint64_t key, uint32_t lane, unsigned long long m_on) {
  const uint32_t key_lo = __shfl_up((uint32_t)key, 1, 64), key_hi = __shfl_up((uint32_t)(key >> 32), 1, 64);
  const bool on_before = lane != 0u && (m_on >> (lane - 1u) & 1ull);
  return on && !(on_before && ((unsigned long long)key_hi << 32 | key_lo) == key);
}

// The cloud that holds `row` of the call's array: the largest c with off[c] <= row (empty clouds share an offset). The
// workgroup's first row is placed by a bisection (uniform, at most 8 steps), a thread walks on from there (a workgroup rarely
// meets a cloud boundary).
__device__ __forceinline__ uint32_t cloud_of_row(const OrgOffsets& offs, uint32_t n_clouds, unsigned long long row_of_block, unsigned long long row) {
  uint32_t lo = 0, hi = n_clouds;
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (offs.off[mid] <= row_of_block) lo = mid;
    else hi = mid;
  }
  uint32_t c = lo;
  while (c + 1u < n_clouds && row >= offs.off[c + 1u]) c++;
  return c;
}

template <typename T>
__device__ __forceinline__ Vec3 load_point_strided(const T* __restrict__ pts, unsigned long long row, uint32_t stride) {
  const T* p = pts + (size_t)row * stride;
  return v3((double)p[0], (double)p[1], (double)p[2]);
}

}  // namespace loamx
