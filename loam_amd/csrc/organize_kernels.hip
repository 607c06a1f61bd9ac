// organize_kernels.hip — unordered clouds into organised scans (loamx.h: loamx_organize_clouds_dev; the rule per point:
// organize_math.h). Two streaming passes over a claim table:
//   classify + claim  one thread per point: load it (3 scalars, point_stride apart), find its cell, claim the cell in the
//                     cloud's table of H W words with an integer atomicMin — the point's index (KEEP_FIRST), or the bits of
//                     its r2 (KEEP_NEAREST; positive doubles order as their bit patterns), after which a second pass over
//                     the points lets those whose r2 IS the cell's minimum claim it with their index. A minimum of integers
//                     does not depend on the order of arrival: that is all the determinism there is to it.
//   gather            one thread per cell: read the winner, copy its three scalars as they are, write the point, its index
//                     and the count of filled cells.
// The two tables (W x 16 B of column directions, (H + 1) x 8 B of tangents) are read through the caches, not staged in LDS: a
// workgroup of 256 points would have to load up to 64 KB to use 12 x 16 B of it per point, and the bisection's first steps hit
// the same few lines from every lane. Algorithmic bytes — per point: 3 scalars read (24 B, 12 B for float clouds; the sector
// the hardware fetches is the whole stride), 2 B of ring number where given, one 4 B atomic (KEEP_NEAREST: one 8 B atomic, 4 B
// cell written and read, the point read again, one more 4 B atomic for the points at their cell's minimum); per cell: 4 B
// (+ 8 B) of table reset, 4 B winner read, 3 scalars read for a filled cell, 3 scalars + 4 B index written.
// The drops are counted per wavefront (ballot, one atomic add by its first lane): integer adds, exact in any order.
#include "loamx_internal.h"

namespace loamx {
namespace {

constexpr int kOrgThreads = 256;
constexpr uint32_t kOrgEmpty = 0xFFFFFFFFu;

__device__ __forceinline__ void org_count(uint32_t* counter, bool flag) {
  const unsigned long long b = __ballot(flag);
  if ((threadIdx.x & 63u) == 0 && b) atomicAdd(counter, (uint32_t)__popcll(b));
}

// blockIdx.y = cloud of the chunk, blockIdx.x = block of 256 points of it (the grid covers the largest cloud: the blocks
// beyond a smaller cloud's end leave at once)
template <typename T, bool kNearest>
__global__ __launch_bounds__(kOrgThreads) void organize_classify_kernel(const T* __restrict__ pts, uint32_t stride, const uint16_t* __restrict__ rings,
                                                                         OrgOffsets offs, OrgTables L, uint32_t* __restrict__ winner,
                                                                         unsigned long long* __restrict__ range, uint32_t* __restrict__ cell_out,
                                                                         uint32_t* __restrict__ counters) {
  const uint32_t c = blockIdx.y;
  const unsigned long long first = offs.off[c], n = offs.off[c + 1] - first;
  const unsigned long long b0 = (unsigned long long)blockIdx.x * kOrgThreads;
  if (b0 >= n) return;
  const unsigned long long i = b0 + threadIdx.x;
  bool invalid = false, outside = false;
  if (i < n) {
    const T* p = pts + (size_t)(first + i) * stride;
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    const uint32_t ring = rings ? (uint32_t)rings[first + i] : kOrgNoRing;
    double r2;
    const uint32_t cell = organize_cell(L, x, y, z, ring, r2);
    invalid = cell == kOrgCellInvalid, outside = cell == kOrgCellOutside;
    if (cell < kOrgCellInvalid) {
      const size_t slot = (size_t)c * L.H * L.W + cell;
      if (kNearest) atomicMin(range + slot, (unsigned long long)__double_as_longlong(r2));
      else atomicMin(winner + slot, (uint32_t)i);
    }
    if (kNearest) cell_out[(size_t)(first - offs.off[0] + i)] = cell;
  }
  org_count(counters + c * kOrgCounterWords + kOrgInvalid, invalid);
  org_count(counters + c * kOrgCounterWords + kOrgOutside, outside);
}

// KEEP_NEAREST, second pass: of the points whose r2 is their cell's minimum the lowest index. r2 is formed again from the
// point by the same function, so it is the same bits.
template <typename T>
__global__ __launch_bounds__(kOrgThreads) void organize_resolve_kernel(const T* __restrict__ pts, uint32_t stride, OrgOffsets offs, uint32_t HW,
                                                                        uint32_t* __restrict__ winner, const unsigned long long* __restrict__ range,
                                                                        const uint32_t* __restrict__ cell_in) {
  const uint32_t c = blockIdx.y;
  const unsigned long long first = offs.off[c], n = offs.off[c + 1] - first;
  const unsigned long long i = (unsigned long long)blockIdx.x * kOrgThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t cell = cell_in[(size_t)(first - offs.off[0] + i)];
  if (cell >= kOrgCellInvalid) return;
  const T* p = pts + (size_t)(first + i) * stride;
  double rho2, r2;
  (void)organize_valid((double)p[0], (double)p[1], (double)p[2], rho2, r2);
  const size_t slot = (size_t)c * HW + cell;
  if ((unsigned long long)__double_as_longlong(r2) == range[slot]) atomicMin(winner + slot, (uint32_t)i);
}

// blockIdx.y = cloud, blockIdx.x = block of 256 cells
template <typename T>
__global__ __launch_bounds__(kOrgThreads) void organize_gather_kernel(const T* __restrict__ pts, uint32_t stride, OrgOffsets offs, uint32_t HW,
                                                                       const uint32_t* __restrict__ winner, T* __restrict__ scans,
                                                                       uint32_t* __restrict__ src_idx, uint32_t* __restrict__ counters) {
  const uint32_t c = blockIdx.y;
  const uint32_t cell = blockIdx.x * kOrgThreads + threadIdx.x;
  bool filled = false;
  if (cell < HW) {
    const size_t slot = (size_t)c * HW + cell;
    const uint32_t w = winner[slot];
    filled = w != kOrgEmpty;
    T v0 = (T)0, v1 = (T)0, v2 = (T)0;
    if (filled) {
      const T* p = pts + (size_t)(offs.off[c] + w) * stride;
      v0 = p[0], v1 = p[1], v2 = p[2];
    }
    T* o = scans + slot * 3;
    o[0] = v0, o[1] = v1, o[2] = v2;
    if (src_idx) src_idx[slot] = w;
  }
  org_count(counters + c * kOrgCounterWords + kOrgFilled, filled);
}

// one thread per cloud: {filled, invalid, outside, collisions = the rest of the cloud}
__global__ __launch_bounds__(kOrgThreads) void organize_stats_kernel(OrgOffsets offs, uint32_t n_clouds, const uint32_t* __restrict__ counters,
                                                                      uint32_t* __restrict__ stats) {
  const uint32_t c = blockIdx.x * kOrgThreads + threadIdx.x;
  if (c >= n_clouds) return;
  const uint32_t n = (uint32_t)(offs.off[c + 1] - offs.off[c]);
  const uint32_t f = counters[c * kOrgCounterWords + kOrgFilled], iv = counters[c * kOrgCounterWords + kOrgInvalid];
  const uint32_t ou = counters[c * kOrgCounterWords + kOrgOutside];
  stats[4 * c] = f, stats[4 * c + 1] = iv, stats[4 * c + 2] = ou, stats[4 * c + 3] = n - f - iv - ou;
}

template <typename T>
void launch_organize_t(const T* pts, uint32_t stride, const uint16_t* d_rings, const OrgOffsets& offs, uint32_t n_clouds, unsigned long long max_points,
                       const OrgTables& L, bool nearest, uint32_t* winner, unsigned long long* range, uint32_t* cell, uint32_t* counters, T* d_scans,
                       uint32_t* d_src_idx, uint32_t* d_stats, hipStream_t s) {
  const uint32_t HW = L.H * L.W;
  const dim3 block(kOrgThreads);
  if (max_points > 0) {
    const dim3 grid((unsigned)((max_points + kOrgThreads - 1) / kOrgThreads), n_clouds);
    if (nearest) {
      launch_kernel((organize_classify_kernel<T, true>), grid, block, 0, s, pts, stride, d_rings, offs, L, winner, range, cell, counters);
      launch_kernel((organize_resolve_kernel<T>), grid, block, 0, s, pts, stride, offs, HW, winner, (const unsigned long long*)range, (const uint32_t*)cell);
    } else {
      launch_kernel((organize_classify_kernel<T, false>), grid, block, 0, s, pts, stride, d_rings, offs, L, winner, range, cell, counters);
    }
  }
  launch_kernel((organize_gather_kernel<T>), dim3((HW + kOrgThreads - 1) / kOrgThreads, n_clouds), block, 0, s, pts, stride, offs, HW,
                (const uint32_t*)winner, d_scans, d_src_idx, counters);
  if (d_stats)
    launch_kernel(organize_stats_kernel, dim3((n_clouds + kOrgThreads - 1) / kOrgThreads), block, 0, s, offs, n_clouds, (const uint32_t*)counters, d_stats);
}

}  // namespace

void launch_organize(const void* d_points, bool f32, uint32_t stride, const uint16_t* d_rings, const OrgOffsets& offs, uint32_t n_clouds,
                     unsigned long long max_points, const OrgTables& L, bool nearest, uint32_t* winner, unsigned long long* range, uint32_t* cell,
                     uint32_t* counters, void* d_scans, uint32_t* d_src_idx, uint32_t* d_stats, hipStream_t s) {
  if (n_clouds == 0) return;
  if (f32)
    launch_organize_t(static_cast<const float*>(d_points), stride, d_rings, offs, n_clouds, max_points, L, nearest, winner, range, cell, counters,
                      static_cast<float*>(d_scans), d_src_idx, d_stats, s);
  else
    launch_organize_t(static_cast<const double*>(d_points), stride, d_rings, offs, n_clouds, max_points, L, nearest, winner, range, cell, counters,
                      static_cast<double*>(d_scans), d_src_idx, d_stats, s);
}

}  // namespace loamx
