// listed_accumulate.h — the accumulate kernel of a listed voxel table (ListedTable of loamx_internal.h), written once for the cloud
// map (cloudmap_kernels.hip) and the surfel map (surfel_kernels.hip). A map supplies a Payload: how many 64-bit words a slot holds
// and how a point fills them. Device only.
#pragma once
#include "cloudmap_math.h"
#include "loamx_internal.h"
#include "voxel_table.h"

namespace loamx {

constexpr int kListedThreads = (int)kMapTile;  // one point or list entry per thread; the tiles of the compaction are the workgroups
constexpr uint32_t kListedCounted = 5;         // words a workgroup counts in LDS: kCloudUsed .. kCloudOutside, then the claims

inline dim3 listed_tiles(unsigned long long n) { return dim3((uint32_t)((n + kMapTile - 1) / kMapTile)); }

__device__ __forceinline__ unsigned long long shfl_down_u64(unsigned long long v, uint32_t d) {
  const uint32_t lo = __shfl_down((uint32_t)v, d, 64), hi = __shfl_down((uint32_t)(v >> 32), d, 64);
  return (unsigned long long)hi << 32 | lo;
}

/* Thread i holds point p0 + i of the call's array; its cloud is cloud_of_row's (voxel_table.h). Validity, p' = pose_c.act(p)
 * with the pose read from device memory, key and offsets as cloudmap_math.h has them, then the kWords words of Payload::point
 *   static __device__ void point(const uint32_t u[3], Vec3 o, Vec3 p, double leaf, unsigned long long m[kWords])
 * (u: the offsets inside the voxel, o: the pose's origin, p: the posed point).
 *
 * kCombine: neighbouring cells of a scan line mostly share a voxel, and one CAS chain plus kWords + 2 atomics per point would then
 * be contention on a few addresses. Lanes that hold the same key in adjacent lanes with a voxel form a run; a run's number is
 * the count of run heads up to its lanes (ballot of the heads, popcount up to the lane), so A B A is three runs whatever the
 * keys say at a distance. A segmented reduction over the run numbers (shifts of 1, 2, 4 ... 32: lane l takes lane l + d's words
 * while that lane has l's run number; runs are contiguous, so what it takes is always the next stretch of its own run) leaves
 * the run's words and its count in the head, which alone claims and issues the atomics. The head has the lowest index of its
 * run, so it alone supplies `first`. A lane without a voxel ends a run; it keeps the number of the run before it, so it must
 * carry zeros: m[] starts as zeros and is written only after cloud_cell has succeeded, so a point that is invalid, dropped by
 * range, or out of range on one axis only holds none. Signed terms travel as two's-complement words: their sums wrap exactly as
 * the signed sums would. All words are integers: combined or not, the table ends up with the same bytes.
 *
 * The claim follows the rule of voxel_table.h (voxel_claim). When the probe gives up, the run's points are counted as overflow
 * and touch nothing else. A head's atomics: the payload words in ascending order, the count, then `first`. slot_out[i]: the slot
 * a head claimed, kMapNoSlot for every other thread. Counters: one atomic per workgroup and word that has something to add; the
 * claims word counts the heads, that is, the CAS chains begun (loamx_cloud_map_claims_read, loamx_surfel_map_claims_read: what
 * tools/bench_cloudmap.py and tools/bench_surfel.py price the two forms with). */
template <typename T, bool kCombine, typename Payload>
__global__ __launch_bounds__(kListedThreads) void listed_accumulate_kernel(const T* __restrict__ pts, uint32_t stride, OrgOffsets offs, uint32_t n_clouds,
                                                                           unsigned long long p0, uint32_t n, uint32_t g0,
                                                                           const double* __restrict__ poses, CloudRule rule, ListedTable t,
                                                                           uint32_t* __restrict__ slot_out) {
  constexpr int kWords = Payload::kWords;
  __shared__ uint32_t s_count[4][kListedCounted];
  const uint32_t i = blockIdx.x * kListedThreads + threadIdx.x, lane = threadIdx.x & 63u;
  const bool in = i < n;
  const unsigned long long row = p0 + i;

  int what = -1;  // kCloud*, -1: no point
  uint64_t key = 0;
  unsigned long long m[kWords];
#pragma unroll
  for (int k = 0; k < kWords; k++) m[k] = 0ull;
  if (in) {
    const uint32_t c = cloud_of_row(offs, n_clouds, p0 + (unsigned long long)blockIdx.x * kListedThreads, row);
    Vec3 p = load_point_strided(pts, row, stride);
    what = cloud_validity(p, rule.min_r2, rule.max_r2);
    if (what == kCloudUsed) {
      Vec3 o = v3(0.0, 0.0, 0.0);
      if (poses) {
        double P[7];
        for (int k = 0; k < 7; k++) P[k] = poses[(size_t)c * 7 + k];
        p = pose_act(P, p);
        o = v3(P[4], P[5], P[6]);
      }
      uint32_t u[3];
      if (cloud_cell(p, rule.leaf, key, u)) Payload::point(u, o, p, rule.leaf, m);
      else what = kCloudOutside;
    }
  }
  const bool ok = what == kCloudUsed;
  const unsigned long long m_ok = __ballot(ok), m_inv = __ballot(what == kCloudInvalid), m_rng = __ballot(what == kCloudRange),
                           m_out = __ballot(what == kCloudOutside);

  uint32_t cnt = ok ? 1u : 0u;
  bool head = ok;
  if (kCombine) {
    head = run_head(ok, key, lane, m_ok);
    const unsigned long long m_head = __ballot(head);
    if (m_head != m_ok) {  // (uniform) some run has more than one lane
      const uint32_t run = (uint32_t)__popcll(m_head & (~0ull >> (63u - lane)));  // heads up to and including this lane
      for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t run_d = __shfl_down(run, d, 64), cnt_d = __shfl_down(cnt, d, 64);
        const bool take = lane + d < 64u && run_d == run;
#pragma unroll
        for (int k = 0; k < kWords; k++) {
          const unsigned long long a = shfl_down_u64(m[k], d);
          if (take) m[k] += a;
        }
        if (take) cnt += cnt_d;
      }
    }
  }

  const unsigned long long m_claim = __ballot(head);
  uint32_t slot = kMapNoSlot;
  bool gave_up = false;
  if (head) {
    bool opened;
    slot = voxel_claim(t.keys, t.log2_cap, key, opened);
    if (slot != kMapNoSlot) {  // slot < 2^log2_cap: the words of the slot start at slot * kWords
      unsigned long long* w = t.payload + (size_t)slot * kWords;
#pragma unroll
      for (int k = 0; k < kWords; k++) atomicAdd(w + k, m[k]);
      atomicAdd(t.count + slot, cnt);
      atomicMin(t.first + slot, g0 + i);
    } else {
      gave_up = true;
      atomicAdd(t.words + kCloudWordOverflow, (unsigned long long)cnt);
    }
  }
  // counters: the wavefronts' ballots meet in LDS, one atomic per workgroup and word that has something to add (an atomic per
  // wavefront on the same few addresses cost more than the rest of the kernel). A wavefront in which a probe gave up adds
  // its used points head by head instead.
  const bool wave_gave_up = __ballot(gave_up) != 0ull;
  if (wave_gave_up && head && !gave_up) atomicAdd(t.words + kCloudUsed, (unsigned long long)cnt);
  if (lane == 0) {
    uint32_t* c = s_count[threadIdx.x >> 6];
    c[kCloudUsed] = wave_gave_up ? 0u : (uint32_t)__popcll(m_ok);
    c[kCloudInvalid] = (uint32_t)__popcll(m_inv), c[kCloudRange] = (uint32_t)__popcll(m_rng), c[kCloudOutside] = (uint32_t)__popcll(m_out);
    c[kListedCounted - 1] = (uint32_t)__popcll(m_claim);
  }
  __syncthreads();
  if (threadIdx.x < kListedCounted) {
    const uint32_t k = threadIdx.x, sum = s_count[0][k] + s_count[1][k] + s_count[2][k] + s_count[3][k];
    if (sum) atomicAdd(t.words + (k == kListedCounted - 1 ? (uint32_t)kCloudWordClaims : k), (unsigned long long)sum);
  }
  if (in) slot_out[i] = slot;
}

// the four forms of the kernel behind a map's launch_*_accumulate
template <typename Payload>
void launch_listed_accumulate(const void* d_points, bool f32, uint32_t stride, const OrgOffsets& offs, uint32_t n_clouds, unsigned long long p0, uint32_t n,
                              uint32_t g0, const double* d_poses, const CloudRule& rule, const ListedTable& t, bool combine, uint32_t* d_slot,
                              hipStream_t s) {
  auto go = [&](auto* pts, auto kernel) {
    launch_kernel(kernel, listed_tiles(n), dim3(kListedThreads), 0, s, pts, stride, offs, n_clouds, p0, n, g0, d_poses, rule, t, d_slot);
  };
  const float* pf = static_cast<const float*>(d_points);
  const double* pd = static_cast<const double*>(d_points);
  if (f32) combine ? go(pf, listed_accumulate_kernel<float, true, Payload>) : go(pf, listed_accumulate_kernel<float, false, Payload>);
  else combine ? go(pd, listed_accumulate_kernel<double, true, Payload>) : go(pd, listed_accumulate_kernel<double, false, Payload>);
}

}  // namespace loamx
