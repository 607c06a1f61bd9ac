// surfel_kernels.hip — the surfel map (loamx.h, "surfel map"): posed clouds accumulated on a voxel grid as integer first and second
// moments plus an integer view sum, the voxel list in order of first appearance, and the records (mean, covariance, eigenvalues,
// oriented normal) read out in that order or looked up per point. Per-point arithmetic and the finish: surfel_math.h; the table:
// voxel_table.h; the stable compaction: map_compact.h.
//
// An add is the cloud map's five launches per chunk of points: accumulate, the flags of the points that opened a voxel, the two
// launches of the compaction's tile offsets, the append to the list, and one thread that commits the list's length. The four small
// list kernels are this unit's own copies of the cloud map's (they differ in the table type only; cloudmap_kernels.hip is left as
// it is). No launch waits for another workgroup, and every loop has a bound that does not depend on the data.
#include "loamx_internal.h"
#include "map_compact.h"
#include "surfel_math.h"
#include "surfel_slot.h"
#include "voxel_table.h"

namespace loamx {
namespace {

static_assert(kSurfelSlotWords == (uint32_t)kSurfelMoments, "a slot holds the twelve words of surfel_point");
static_assert(sizeof(loamx_surfel) == 128, "loamx_surfel is 128 bytes");

constexpr int kSurfelThreads = (int)kMapTile;  // one point per thread; the tiles of the compaction are the workgroups
constexpr uint32_t kSurfelCounted = 5;         // words a workgroup counts in LDS: kCloudUsed .. kCloudOutside, then the claims

__device__ __forceinline__ unsigned long long shfl_down_u64(unsigned long long v, uint32_t d) {
  const uint32_t lo = __shfl_down((uint32_t)v, d, 64), hi = __shfl_down((uint32_t)(v >> 32), d, 64);
  return (unsigned long long)hi << 32 | lo;
}

/* ---- accumulate ----------------------------------------------------------------------------------------------------
 * The shape of cloud_accumulate_kernel (cloudmap_kernels.hip): thread i holds point p0 + i of the call's array, its cloud is
 * cloud_of_row's; validity, p' = pose_c.act(p), key and offsets as cloudmap_math.h has them, then the twelve words of
 * surfel_point. A head issues one CAS chain, twelve 64-bit atomicAdd, one 32-bit add and one atomicMin: 14 atomics against the
 * cloud map's 5, which is what run combining saves per combined lane.
 *
 * kCombine: runs as run_head (voxel_table.h) defines them, and the cloud map's segmented reduction over the run numbers, here
 * over thirteen values. A lane without a voxel keeps the number of the run before it, so it carries zeros in all thirteen, the
 * signed view terms included (forced below). The view terms travel as two's-complement words: their sums wrap exactly as the
 * signed sums would, and |W| < 2^62 by the clamp. All sums are integers: combined or not, the table ends up with the same bytes.
 *
 * The claim follows the rule of voxel_table.h. When the probe gives up, the run's points are counted as overflow and touch nothing
 * else. slot_out[i]: the slot a head claimed, kMapNoSlot for every other thread. Counters: the wavefronts' ballots meet in LDS,
 * one atomic per workgroup and word that has something to add; the claims word counts the heads. */
template <typename T, bool kCombine>
__global__ __launch_bounds__(kSurfelThreads) void surfel_accumulate_kernel(const T* __restrict__ pts, uint32_t stride, OrgOffsets offs, uint32_t n_clouds,
                                                                           unsigned long long p0, uint32_t n, uint32_t g0,
                                                                           const double* __restrict__ poses, CloudRule rule, SurfelTable t,
                                                                           uint32_t* __restrict__ slot_out) {
  __shared__ uint32_t s_count[4][kSurfelCounted];
  const uint32_t i = blockIdx.x * kSurfelThreads + threadIdx.x, lane = threadIdx.x & 63u;
  const bool in = i < n;
  const unsigned long long row = p0 + i;

  int what = -1;  // kCloud*, -1: no point
  uint64_t key = 0;
  unsigned long long m[kSurfelMoments];
#pragma unroll
  for (int k = 0; k < kSurfelMoments; k++) m[k] = 0ull;
  if (in) {
    const uint32_t c = cloud_of_row(offs, n_clouds, p0 + (unsigned long long)blockIdx.x * kSurfelThreads, row);
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
      if (cloud_cell(p, rule.leaf, key, u)) surfel_point(u, o, p, rule.leaf, m);
      else what = kCloudOutside;
    }
  }
  const bool ok = what == kCloudUsed;
  const unsigned long long m_ok = __ballot(ok), m_inv = __ballot(what == kCloudInvalid), m_rng = __ballot(what == kCloudRange),
                           m_out = __ballot(what == kCloudOutside);

  // (m is written only for a point with a voxel: every other lane still holds the zeros it must carry)
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
        for (int k = 0; k < kSurfelMoments; k++) {
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
    if (slot != kMapNoSlot) {  // slot < 2^log2_cap: the twelve words of the slot start at slot * kSurfelSlotWords
      unsigned long long* w = t.mom + (size_t)slot * kSurfelSlotWords;
#pragma unroll
      for (int k = 0; k < kSurfelMoments; k++) atomicAdd(w + k, m[k]);
      atomicAdd(t.count + slot, cnt);
      atomicMin(t.first + slot, g0 + i);
    } else {
      gave_up = true;
      atomicAdd(t.words + kCloudWordOverflow, (unsigned long long)cnt);
    }
  }
  // counters as in cloud_accumulate_kernel: a wavefront in which a probe gave up adds its used points head by head instead
  const bool wave_gave_up = __ballot(gave_up) != 0ull;
  if (wave_gave_up && head && !gave_up) atomicAdd(t.words + kCloudUsed, (unsigned long long)cnt);
  if (lane == 0) {
    uint32_t* c = s_count[threadIdx.x >> 6];
    c[kCloudUsed] = wave_gave_up ? 0u : (uint32_t)__popcll(m_ok);
    c[kCloudInvalid] = (uint32_t)__popcll(m_inv), c[kCloudRange] = (uint32_t)__popcll(m_rng), c[kCloudOutside] = (uint32_t)__popcll(m_out);
    c[kSurfelCounted - 1] = (uint32_t)__popcll(m_claim);
  }
  __syncthreads();
  if (threadIdx.x < kSurfelCounted) {
    const uint32_t k = threadIdx.x, sum = s_count[0][k] + s_count[1][k] + s_count[2][k] + s_count[3][k];
    if (sum) atomicAdd(t.words + (k == kSurfelCounted - 1 ? (uint32_t)kCloudWordClaims : k), (unsigned long long)sum);
  }
  if (in) slot_out[i] = slot;
}

/* ---- list upkeep: the cloud map's scheme (new-voxel flags from `first`, tile offsets, append, commit) ---------------------- */
// point g opened its voxel iff the voxel's `first` is g (plain loads are fine across the kernel boundary)
__global__ __launch_bounds__(kSurfelThreads) void surfel_new_flags_kernel(const uint32_t* __restrict__ first, const uint32_t* __restrict__ slot,
                                                                          uint32_t n, uint32_t g0, uint8_t* __restrict__ keep) {
  const uint32_t i = blockIdx.x * kSurfelThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = slot[i];
  keep[i] = s != kMapNoSlot && first[s] == g0 + i;
}

// the flagged points' slots behind the list's present end, in input order; what does not fit is counted, never written
__global__ __launch_bounds__(kSurfelThreads) void surfel_append_kernel(const uint8_t* __restrict__ keep, const uint32_t* __restrict__ slot, uint32_t n,
                                                                       const uint32_t* __restrict__ tiles, SurfelTable t) {
  __shared__ uint32_t s_wave[4];
  const uint32_t i = blockIdx.x * kSurfelThreads + threadIdx.x;
  const bool flag = i < n && keep[i] != 0;
  uint32_t total;
  const uint32_t rank = block_rank(flag, s_wave, total);
  if (!flag) return;
  const unsigned long long dst = (unsigned long long)t.lens[kCloudLenListed] + tiles[blockIdx.x] + rank;
  if (dst < t.max_voxels) t.list[dst] = slot[i];
  else atomicAdd(t.words + kCloudWordOverflow, 1ull);
}

// one thread, behind the append: the list has grown by the chunk's new voxels (those that fitted)
__global__ void surfel_commit_kernel(SurfelTable t) {
  const unsigned long long len = (unsigned long long)t.lens[kCloudLenListed] + t.lens[kCloudLenPending];
  t.lens[kCloudLenListed] = len < t.max_voxels ? (uint32_t)len : t.max_voxels;
}

/* ---- read-outs ---------------------------------------------------------------------------------------------------------------- */
// (the record of a slot: surfel_of_slot of surfel_slot.h)
// one thread per list entry up to the list's capacity (its length is known on the device only)
__global__ __launch_bounds__(kSurfelThreads) void surfel_emit_flags_kernel(SurfelTable t, uint32_t min_points, uint8_t* __restrict__ keep) {
  const uint32_t j = blockIdx.x * kSurfelThreads + threadIdx.x;
  if (j >= t.max_voxels) return;
  keep[j] = j < t.lens[kCloudLenListed] && t.count[t.list[j]] >= min_points;
}

// one listed voxel per thread, surfel_finish in registers, one 128-byte record out (and the mean and the normal on their own)
__global__ __launch_bounds__(kSurfelThreads) void surfel_emit_scatter_kernel(const uint8_t* __restrict__ keep, const uint32_t* __restrict__ tiles,
                                                                             SurfelTable t, double leaf, unsigned long long capacity,
                                                                             loamx_surfel* __restrict__ out, double* __restrict__ xyz_out,
                                                                             double* __restrict__ normal_out) {
  __shared__ uint32_t s_wave[4];
  const uint32_t j = blockIdx.x * kSurfelThreads + threadIdx.x;
  const bool flag = j < t.max_voxels && keep[j] != 0;
  uint32_t total;
  const uint32_t rank = block_rank(flag, s_wave, total);
  if (!flag) return;
  const uint32_t dst = tiles[blockIdx.x] + rank;
  if (dst >= capacity) return;
  const uint32_t s = t.list[j];
  const loamx_surfel r = surfel_of_slot(t, s, t.count[s], leaf);
  if (out) out[dst] = r;
  if (xyz_out)
    for (int a = 0; a < 3; a++) xyz_out[(size_t)dst * 3 + a] = r.mean[a];
  if (normal_out)
    for (int a = 0; a < 3; a++) normal_out[(size_t)dst * 3 + a] = r.normal[a];
}

// one point per thread: its voxel by cloud_cell at the map's leaf, voxel_find by plain loads (behind the adds on the same stream:
// a kernel boundary, as the rule of the table requires), surfel_finish, the signed distance
__global__ __launch_bounds__(kSurfelThreads) void surfel_query_kernel(SurfelTable t, double leaf, uint32_t min_points, const double* __restrict__ pts,
                                                                      uint32_t stride, unsigned long long n, loamx_surfel* __restrict__ out,
                                                                      double* __restrict__ distance_out, uint32_t* __restrict__ count_out) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kSurfelThreads + threadIdx.x;
  if (i >= n) return;
  const Vec3 p = load_point_strided(pts, i, stride);
  uint64_t key = 0;
  uint32_t u[3];
  uint32_t s = kMapNoSlot, cnt = 0;
  if (cloud_cell(p, leaf, key, u)) s = voxel_find(t.keys, t.log2_cap, key);
  if (s != kMapNoSlot) cnt = t.count[s];
  loamx_surfel r;
  double dist = 0.0;
  if (s != kMapNoSlot && cnt != 0u && cnt >= min_points) {
    r = surfel_of_slot(t, s, cnt, leaf);
    dist = surfel_distance(r, p);
  } else {
    for (int a = 0; a < 3; a++) r.mean[a] = 0.0, r.eval[a] = 0.0, r.normal[a] = 0.0;
    for (int a = 0; a < 6; a++) r.cov[a] = 0.0;
    r.count = 0u, r.first = 0u;
    cnt = 0u;
  }
  if (out) out[i] = r;
  if (distance_out) distance_out[i] = dist;
  if (count_out) count_out[i] = cnt;
}

inline dim3 surfel_tiles(unsigned long long n) { return dim3((uint32_t)((n + kMapTile - 1) / kMapTile)); }

template <typename T, bool kCombine>
void accumulate(const void* d_points, uint32_t stride, const OrgOffsets& offs, uint32_t n_clouds, unsigned long long p0, uint32_t n, uint32_t g0,
                const double* d_poses, const CloudRule& rule, const SurfelTable& t, uint32_t* d_slot, hipStream_t s) {
  launch_kernel((surfel_accumulate_kernel<T, kCombine>), surfel_tiles(n), dim3(kSurfelThreads), 0, s, static_cast<const T*>(d_points), stride, offs,
                n_clouds, p0, n, g0, d_poses, rule, t, d_slot);
}

}  // namespace

// Points p0 .. p0 + n - 1 of the call's array (0 < n <= kCloudChunkPoints), which lie in the clouds of `offs`; g0: the running
// index of point p0; d_poses: the pose of offs' first cloud onwards, or nullptr. d_slot: n words.
void launch_surfel_accumulate(const void* d_points, bool f32, uint32_t stride, const OrgOffsets& offs, uint32_t n_clouds, unsigned long long p0,
                              uint32_t n, uint32_t g0, const double* d_poses, const CloudRule& rule, const SurfelTable& t, bool combine, uint32_t* d_slot,
                              hipStream_t s) {
  if (f32) {
    if (combine) accumulate<float, true>(d_points, stride, offs, n_clouds, p0, n, g0, d_poses, rule, t, d_slot, s);
    else accumulate<float, false>(d_points, stride, offs, n_clouds, p0, n, g0, d_poses, rule, t, d_slot, s);
  } else {
    if (combine) accumulate<double, true>(d_points, stride, offs, n_clouds, p0, n, g0, d_poses, rule, t, d_slot, s);
    else accumulate<double, false>(d_points, stride, offs, n_clouds, p0, n, g0, d_poses, rule, t, d_slot, s);
  }
}

// behind launch_surfel_accumulate of the same points: their new voxels join the list. d_keep: n bytes; d_tiles: map_compact_ws_bytes(n)
void launch_surfel_list(const SurfelTable& t, const uint32_t* d_slot, uint32_t n, uint32_t g0, uint8_t* d_keep, uint32_t* d_tiles, hipStream_t s) {
  launch_kernel(surfel_new_flags_kernel, surfel_tiles(n), dim3(kSurfelThreads), 0, s, (const uint32_t*)t.first, d_slot, n, g0, d_keep);
  launch_tile_offsets(d_keep, n, d_tiles, t.lens + kCloudLenPending, s);
  launch_kernel(surfel_append_kernel, surfel_tiles(n), dim3(kSurfelThreads), 0, s, (const uint8_t*)d_keep, d_slot, n, (const uint32_t*)d_tiles, t);
  launch_kernel(surfel_commit_kernel, dim3(1), dim3(1), 0, s, t);
}

// d_keep: max_voxels bytes; d_tiles: map_compact_ws_bytes(max_voxels). Writes *d_n_out in every case.
void launch_surfel_emit(const SurfelTable& t, double leaf, uint32_t min_points, uint8_t* d_keep, uint32_t* d_tiles, loamx_surfel* d_out,
                        double* d_xyz_out, double* d_normal_out, size_t capacity, uint32_t* d_n_out, hipStream_t s) {
  launch_kernel(surfel_emit_flags_kernel, surfel_tiles(t.max_voxels), dim3(kSurfelThreads), 0, s, t, min_points, d_keep);
  launch_tile_offsets(d_keep, t.max_voxels, d_tiles, d_n_out, s);
  if (capacity == 0 || (!d_out && !d_xyz_out && !d_normal_out)) return;  // (only the number was asked for)
  launch_kernel(surfel_emit_scatter_kernel, surfel_tiles(t.max_voxels), dim3(kSurfelThreads), 0, s, (const uint8_t*)d_keep, (const uint32_t*)d_tiles, t,
                leaf, (unsigned long long)capacity, d_out, d_xyz_out, d_normal_out);
}

void launch_surfel_query(const SurfelTable& t, double leaf, uint32_t min_points, const double* d_points, uint32_t stride, unsigned long long n,
                         loamx_surfel* d_out, double* d_distance_out, uint32_t* d_count_out, hipStream_t s) {
  if (n == 0 || (!d_out && !d_distance_out && !d_count_out)) return;
  launch_kernel(surfel_query_kernel, surfel_tiles(n), dim3(kSurfelThreads), 0, s, t, leaf, min_points, d_points, stride, n, d_out, d_distance_out,
                d_count_out);
}

}  // namespace loamx
