// cloudmap_kernels.hip — the cloud map (loamx.h, "cloud map"): posed clouds accumulated on a voxel grid as integer sums, the
// voxel list in order of first appearance, and the centroids read out in that order. Per-point arithmetic: cloudmap_math.h;
// the stable compaction is the one of map_kernels.hip (map_compact.h).
//
// An add is five launches per chunk of points: accumulate (below), the flags of the points that opened a voxel, the two
// launches of the compaction's tile offsets, the append of the flagged points' slots to the list, and one thread that adds
// the chunk's new voxels to the list's length. An emit is flags over the list, the tile offsets, and a scatter that forms
// the centroids. No launch waits for another workgroup, and every loop has a bound that does not depend on the data.
#include "cloudmap_math.h"
#include "loamx_internal.h"
#include "map_compact.h"
#include "voxel_table.h"

namespace loamx {
namespace {

constexpr int kCloudThreads = (int)kMapTile;  // one point per thread; the tiles of the compaction are the workgroups
constexpr uint32_t kCloudCounted = 5;         // words a workgroup counts in LDS: kCloudUsed .. kCloudOutside, then the claims

__device__ __forceinline__ unsigned long long shfl_down_u64(unsigned long long v, uint32_t d) {
  const uint32_t lo = __shfl_down((uint32_t)v, d, 64), hi = __shfl_down((uint32_t)(v >> 32), d, 64);
  return (unsigned long long)hi << 32 | lo;
}

/* ---- accumulate ----------------------------------------------------------------------------------------------------
 * Thread i holds point p0 + i of the call's array; its cloud is cloud_of_row's (voxel_table.h). Validity, p' = pose_c.act(p)
 * with the pose read from device memory, key and offsets as cloudmap_math.h has them.
 *
 * kCombine: neighbouring cells of a scan line mostly share a voxel, and one CAS chain plus five atomics per point would then
 * be contention on a few addresses. Lanes that hold the same key in adjacent lanes with a voxel form a run; a run's number is
 * the count of run heads up to its lanes (ballot of the heads, popcount up to the lane), so A B A is three runs whatever the
 * keys say at a distance. A segmented reduction over the run numbers (shifts of 1, 2, 4 ... 32: lane l takes lane l + d's sums
 * while that lane has l's run number; runs are contiguous, so what it takes is always the next stretch of its own run) leaves
 * the run's three sums and its count in the head, which alone claims and issues the atomics. The head has the lowest index
 * of its run, so it alone supplies `first`. A lane without a voxel ends a run; it keeps the number of the run before it, so
 * it must carry zeros (they are forced below, also for a point whose voxel is out of range on one axis only). The sums are integers:
 * combined or not, the table ends up with the same bytes.
 *
 * The claim follows the rule of voxel_table.h (voxel_claim). When the probe gives up, the run's points are counted as overflow
 * and touch nothing else. slot_out[i]: the slot a head claimed, kMapNoSlot for every
 * other thread. Counters: one atomic per workgroup and word that has something to add; the claims word counts the heads, that
 * is, the CAS chains begun (loamx_cloud_map_claims_read: what tools/bench_cloudmap.py prices the two forms with). */
template <typename T, bool kCombine>
__global__ __launch_bounds__(kCloudThreads) void cloud_accumulate_kernel(const T* __restrict__ pts, uint32_t stride, OrgOffsets offs, uint32_t n_clouds,
                                                                         unsigned long long p0, uint32_t n, uint32_t g0,
                                                                         const double* __restrict__ poses, CloudRule rule, CloudTable t,
                                                                         uint32_t* __restrict__ slot_out) {
  __shared__ uint32_t s_count[4][kCloudCounted];
  const uint32_t i = blockIdx.x * kCloudThreads + threadIdx.x, lane = threadIdx.x & 63u;
  const bool in = i < n;
  const unsigned long long row = p0 + i;

  int what = -1;  // kCloud*, -1: no point
  uint64_t key = 0;
  uint32_t u[3] = {0u, 0u, 0u};
  if (in) {
    const uint32_t c = cloud_of_row(offs, n_clouds, p0 + (unsigned long long)blockIdx.x * kCloudThreads, row);
    Vec3 p = load_point_strided(pts, row, stride);
    what = cloud_validity(p, rule.min_r2, rule.max_r2);
    if (what == kCloudUsed) {
      if (poses) {
        double P[7];
        for (int k = 0; k < 7; k++) P[k] = poses[(size_t)c * 7 + k];
        p = pose_act(P, p);
      }
      if (!cloud_cell(p, rule.leaf, key, u)) what = kCloudOutside;
    }
  }
  const bool ok = what == kCloudUsed;
  const unsigned long long m_ok = __ballot(ok), m_inv = __ballot(what == kCloudInvalid), m_rng = __ballot(what == kCloudRange),
                           m_out = __ballot(what == kCloudOutside);

  // a lane without a voxel carries the run number of the run before it, so whatever it held would reach that run's head:
  // it carries zeros (cloud_cell leaves none for a point out of range; invalid and range-dropped points never had any)
  unsigned long long s0 = ok ? u[0] : 0u, s1 = ok ? u[1] : 0u, s2 = ok ? u[2] : 0u;
  uint32_t cnt = ok ? 1u : 0u;
  bool head = ok;
  if (kCombine) {
    head = run_head(ok, key, lane, m_ok);
    const unsigned long long m_head = __ballot(head);
    if (m_head != m_ok) {  // (uniform) some run has more than one lane
      const uint32_t run = (uint32_t)__popcll(m_head & (~0ull >> (63u - lane)));  // heads up to and including this lane
      for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t run_d = __shfl_down(run, d, 64), cnt_d = __shfl_down(cnt, d, 64);
        const unsigned long long a0 = shfl_down_u64(s0, d), a1 = shfl_down_u64(s1, d), a2 = shfl_down_u64(s2, d);
        if (lane + d < 64u && run_d == run) s0 += a0, s1 += a1, s2 += a2, cnt += cnt_d;
      }
    }
  }

  const unsigned long long m_claim = __ballot(head);
  uint32_t slot = kMapNoSlot;
  bool gave_up = false;
  if (head) {
    bool opened;
    slot = voxel_claim(t.keys, t.log2_cap, key, opened);
    if (slot != kMapNoSlot) {
      atomicAdd(t.sums + (size_t)slot * 3, s0);
      atomicAdd(t.sums + (size_t)slot * 3 + 1, s1);
      atomicAdd(t.sums + (size_t)slot * 3 + 2, s2);
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
    c[kCloudCounted - 1] = (uint32_t)__popcll(m_claim);
  }
  __syncthreads();
  if (threadIdx.x < kCloudCounted) {
    const uint32_t k = threadIdx.x, sum = s_count[0][k] + s_count[1][k] + s_count[2][k] + s_count[3][k];
    if (sum) atomicAdd(t.words + (k == kCloudCounted - 1 ? (uint32_t)kCloudWordClaims : k), (unsigned long long)sum);
  }
  if (in) slot_out[i] = slot;
}

// second launch (plain loads are fine across the kernel boundary): point g opened its voxel iff the voxel's `first` is g. A
// voxel that existed before the chunk has a smaller `first`, so this is also "the voxel did not exist before the call".
__global__ __launch_bounds__(kCloudThreads) void cloud_new_flags_kernel(const uint32_t* __restrict__ first, const uint32_t* __restrict__ slot, uint32_t n,
                                                                        uint32_t g0, uint8_t* __restrict__ keep) {
  const uint32_t i = blockIdx.x * kCloudThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = slot[i];
  keep[i] = s != kMapNoSlot && first[s] == g0 + i;
}

// the flagged points' slots behind the list's present end, in input order; what does not fit is counted, never written
__global__ __launch_bounds__(kCloudThreads) void cloud_append_kernel(const uint8_t* __restrict__ keep, const uint32_t* __restrict__ slot, uint32_t n,
                                                                     const uint32_t* __restrict__ tiles, CloudTable t) {
  __shared__ uint32_t s_wave[4];
  const uint32_t i = blockIdx.x * kCloudThreads + threadIdx.x;
  const bool flag = i < n && keep[i] != 0;
  uint32_t total;
  const uint32_t rank = block_rank(flag, s_wave, total);
  if (!flag) return;
  const unsigned long long dst = (unsigned long long)t.lens[kCloudLenListed] + tiles[blockIdx.x] + rank;
  if (dst < t.max_voxels) t.list[dst] = slot[i];
  else atomicAdd(t.words + kCloudWordOverflow, 1ull);
}

// one thread, behind the append: the list has grown by the chunk's new voxels (those that fitted)
__global__ void cloud_commit_kernel(CloudTable t) {
  const unsigned long long len = (unsigned long long)t.lens[kCloudLenListed] + t.lens[kCloudLenPending];
  t.lens[kCloudLenListed] = len < t.max_voxels ? (uint32_t)len : t.max_voxels;
}

/* ---- emit ------------------------------------------------------------------------------------------------------------- */
// one thread per list entry up to the list's capacity (its length is known on the device only)
__global__ __launch_bounds__(kCloudThreads) void cloud_emit_flags_kernel(CloudTable t, uint32_t min_points, uint8_t* __restrict__ keep) {
  const uint32_t j = blockIdx.x * kCloudThreads + threadIdx.x;
  if (j >= t.max_voxels) return;
  keep[j] = j < t.lens[kCloudLenListed] && t.count[t.list[j]] >= min_points;
}

__global__ __launch_bounds__(kCloudThreads) void cloud_emit_scatter_kernel(const uint8_t* __restrict__ keep, const uint32_t* __restrict__ tiles, CloudTable t,
                                                                           double leaf, unsigned long long capacity, double* __restrict__ xyz_out,
                                                                           uint32_t* __restrict__ count_out, uint32_t* __restrict__ first_out) {
  __shared__ uint32_t s_wave[4];
  const uint32_t j = blockIdx.x * kCloudThreads + threadIdx.x;
  const bool flag = j < t.max_voxels && keep[j] != 0;
  uint32_t total;
  const uint32_t rank = block_rank(flag, s_wave, total);
  if (!flag) return;
  const uint32_t dst = tiles[blockIdx.x] + rank;
  if (dst >= capacity) return;
  const uint32_t s = t.list[j], cnt = t.count[s];
  const uint64_t key = t.keys[s];
  for (int a = 0; a < 3; a++) xyz_out[(size_t)dst * 3 + a] = cloud_centroid(cloud_key_coord(key, a), t.sums[(size_t)s * 3 + a], cnt, leaf);
  if (count_out) count_out[dst] = cnt;
  if (first_out) first_out[dst] = t.first[s];
}

inline dim3 cloud_tiles(uint32_t n) { return dim3((n + kMapTile - 1) / kMapTile); }

template <typename T, bool kCombine>
void accumulate(const void* d_points, uint32_t stride, const OrgOffsets& offs, uint32_t n_clouds, unsigned long long p0, uint32_t n, uint32_t g0,
                const double* d_poses, const CloudRule& rule, const CloudTable& t, uint32_t* d_slot, hipStream_t s) {
  launch_kernel((cloud_accumulate_kernel<T, kCombine>), cloud_tiles(n), dim3(kCloudThreads), 0, s, static_cast<const T*>(d_points), stride, offs, n_clouds,
                p0, n, g0, d_poses, rule, t, d_slot);
}

}  // namespace

// Points p0 .. p0 + n - 1 of the call's array (0 < n <= kCloudChunkPoints), which lie in the clouds of `offs`; g0: the running
// index of point p0; d_poses: the pose of offs' first cloud onwards, or nullptr. d_slot: n words.
void launch_cloud_accumulate(const void* d_points, bool f32, uint32_t stride, const OrgOffsets& offs, uint32_t n_clouds, unsigned long long p0,
                             uint32_t n, uint32_t g0, const double* d_poses, const CloudRule& rule, const CloudTable& t, bool combine, uint32_t* d_slot,
                             hipStream_t s) {
  if (f32) {
    if (combine) accumulate<float, true>(d_points, stride, offs, n_clouds, p0, n, g0, d_poses, rule, t, d_slot, s);
    else accumulate<float, false>(d_points, stride, offs, n_clouds, p0, n, g0, d_poses, rule, t, d_slot, s);
  } else {
    if (combine) accumulate<double, true>(d_points, stride, offs, n_clouds, p0, n, g0, d_poses, rule, t, d_slot, s);
    else accumulate<double, false>(d_points, stride, offs, n_clouds, p0, n, g0, d_poses, rule, t, d_slot, s);
  }
}

// behind launch_cloud_accumulate of the same points: their new voxels join the list. d_keep: n bytes; d_tiles: map_compact_ws_bytes(n)
void launch_cloud_list(const CloudTable& t, const uint32_t* d_slot, uint32_t n, uint32_t g0, uint8_t* d_keep, uint32_t* d_tiles, hipStream_t s) {
  launch_kernel(cloud_new_flags_kernel, cloud_tiles(n), dim3(kCloudThreads), 0, s, (const uint32_t*)t.first, d_slot, n, g0, d_keep);
  launch_tile_offsets(d_keep, n, d_tiles, t.lens + kCloudLenPending, s);
  launch_kernel(cloud_append_kernel, cloud_tiles(n), dim3(kCloudThreads), 0, s, (const uint8_t*)d_keep, d_slot, n, (const uint32_t*)d_tiles, t);
  launch_kernel(cloud_commit_kernel, dim3(1), dim3(1), 0, s, t);
}

// d_keep: max_voxels bytes; d_tiles: map_compact_ws_bytes(max_voxels). Writes *d_n_out in every case.
void launch_cloud_emit(const CloudTable& t, double leaf, uint32_t min_points, uint8_t* d_keep, uint32_t* d_tiles, double* d_xyz_out,
                       uint32_t* d_count_out, uint32_t* d_first_out, size_t capacity, uint32_t* d_n_out, hipStream_t s) {
  launch_kernel(cloud_emit_flags_kernel, cloud_tiles(t.max_voxels), dim3(kCloudThreads), 0, s, t, min_points, d_keep);
  launch_tile_offsets(d_keep, t.max_voxels, d_tiles, d_n_out, s);
  launch_kernel(cloud_emit_scatter_kernel, cloud_tiles(t.max_voxels), dim3(kCloudThreads), 0, s, (const uint8_t*)d_keep, (const uint32_t*)d_tiles, t, leaf,
                (unsigned long long)capacity, d_xyz_out, d_count_out, d_first_out);
}

}  // namespace loamx
