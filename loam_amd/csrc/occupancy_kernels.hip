// occupancy_kernels.hip — the occupancy map (loamx.h, "occupancy map"): every beam of posed clouds walked through a voxel grid from
// the sensor to its return, two integer counts per voxel (hits, passes) in an open-addressed table, and the three read-outs
// (points, a dense box, a 2-D slice). Per-ray arithmetic: occupancy_math.h. Counts are integer sums and the walk of a ray depends
// on that ray alone: every schedule, every split over workgroups and every batch split leaves the same bytes. No launch waits for
// another workgroup, and every loop has a bound that is known before it starts.
#include "loamx_internal.h"
#include "occupancy_read.h"
#include "voxel_table.h"

namespace loamx {
namespace {

constexpr int kOccThreads = 256;
constexpr uint32_t kOccCounted = 8;  // words a workgroup counts in LDS: kOccWordHit .. kOccWordClaims

/* One visit per lane (or none): `unit` is added to the count word of `key`, 1 for a pass and 2^32 for a hit.
 *
 * The claim follows the rule of voxel_table.h (voxel_claim), and ONE 64-bit atomicAdd follows. When the probe gives up, the
 * visits it stood for are counted as overflow and touch nothing else.
 *
 * kCombine: the lanes of a wavefront are neighbouring beams, and near the sensor their walks stand in the same voxel step after
 * step. Lanes that hold the same key in adjacent lanes with a visit form a run (A B A is three runs); the head of a run alone
 * claims and adds unit x the run's length. Runs are contiguous, so the segmented sum of ones that the cloud map takes by
 * shuffles is here a closed form on the two ballots: a run ends in front of the next head or the next lane without a visit.
 * Integer sums: combined or not, the table ends up with the same bytes. The counts returned are wave-uniform. */
template <bool kCombine>
__device__ __forceinline__ void occ_emit(bool on, uint64_t key, unsigned long long unit, uint32_t lane, const OccTable& t, uint32_t& n_visits,
                                         uint32_t& n_claims, uint32_t& n_won) {
  const unsigned long long m_on = __ballot(on);
  if (m_on == 0ull) return;  // (uniform)
  n_visits += (uint32_t)__popcll(m_on);
  bool head = on;
  uint32_t cnt = 1u;
  if (kCombine) {
    head = run_head(on, key, lane, m_on);
    const unsigned long long m_head = __ballot(head);
    const unsigned long long above = lane == 63u ? 0ull : ~0ull << (lane + 1u);
    const unsigned long long stop = (m_head | ~m_on) & above;
    cnt = (stop ? (uint32_t)__builtin_ctzll(stop) : 64u) - lane;
  }
  n_claims += (uint32_t)__popcll(__ballot(head));
  bool won = false;
  if (head) {
    const uint32_t s = voxel_claim(t.keys, t.log2_cap, key, won);
    if (s != kMapNoSlot) atomicAdd(t.counts + s, unit * cnt);
    else atomicAdd(t.words + kOccWordOverflow, (unsigned long long)cnt);
  }
  n_won += (uint32_t)__popcll(__ballot(won));
}

/* ---- walk -------------------------------------------------------------------------------------------------------------------
 * Thread i holds ray p0 + i of the call's array; its cloud is cloud_of_row's (voxel_table.h). Steps 1 to 4 of the rule up to the
 * walk's first voxel are occ_ray's. The hit goes through occ_emit first, then the wavefront loops while any lane has a voxel left to visit: a lane whose voxel is its
 * own hit voxel, or that has finished, takes no part in that step's runs. The length of every lane's walk is known before the loop
 * starts. Counters: ballots summed per wavefront in uniform registers, met in LDS, one atomic per workgroup and word that has
 * something to add. */
template <typename T, bool kCombine>
__global__ __launch_bounds__(kOccThreads) void occupancy_walk_kernel(const T* __restrict__ pts, uint32_t stride, OrgOffsets offs, uint32_t n_clouds,
                                                                     unsigned long long p0, uint32_t n, const double* __restrict__ poses, OccRule rule,
                                                                     OccTable t) {
  __shared__ uint32_t s_count[kOccThreads / 64][kOccCounted];
  const uint32_t i = blockIdx.x * kOccThreads + threadIdx.x, lane = threadIdx.x & 63u;
  const unsigned long long row = p0 + i;

  OccRay r;
  r.kind = -1, r.has_hit = r.outside = r.walks = false, r.hit_key = 0;
  r.w = OccWalk{};  // (a lane without a walk still forms a key in the loop below; it takes no part, but it reads no indeterminate value)
  if (i < n) {
    const uint32_t c = cloud_of_row(offs, n_clouds, p0 + (unsigned long long)blockIdx.x * kOccThreads, row);
    const Vec3 p = load_point_strided(pts, row, stride);
    double P[7] = {0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    if (poses) {
#pragma unroll
      for (int k = 0; k < 7; k++) P[k] = poses[(size_t)c * 7 + k];
    }
    occ_ray(p, poses != nullptr, P, rule, r);
  }
  const unsigned long long m_inv = __ballot(r.kind == kOccRayInvalid), m_short = __ballot(r.kind == kOccRayShort),
                           m_long = __ballot(r.kind == kOccRayLong), m_out = __ballot(r.outside), m_hit = __ballot(r.has_hit);

  uint32_t n_visits = 0, n_claims = 0, n_won = 0, unused = 0;
  occ_emit<kCombine>(r.has_hit, r.hit_key, kOccHitUnit, lane, t, unused, n_claims, n_won);
  uint32_t left = r.walks ? occ_walk_steps(r.w) + 1u : 0u;  // voxels this lane has still to visit
  while (__ballot(left != 0u) != 0ull) {
    const uint64_t key = occ_walk_key(r.w);
    occ_emit<kCombine>(left != 0u && !(r.has_hit && key == r.hit_key), key, 1ull, lane, t, n_visits, n_claims, n_won);
    if (left != 0u && --left != 0u) occ_walk_step(r.w);
  }

  if (lane == 0) {
    uint32_t* c = s_count[threadIdx.x >> 6];
    c[kOccWordHit] = (uint32_t)__popcll(m_hit), c[kOccWordInvalid] = (uint32_t)__popcll(m_inv), c[kOccWordShort] = (uint32_t)__popcll(m_short);
    c[kOccWordLong] = (uint32_t)__popcll(m_long), c[kOccWordOutside] = (uint32_t)__popcll(m_out);
    c[kOccWordVisits] = n_visits, c[kOccWordVoxels] = n_won, c[kOccWordClaims] = n_claims;
  }
  __syncthreads();
  if (threadIdx.x < kOccCounted) {
    unsigned long long sum = 0;
    for (int w = 0; w < kOccThreads / 64; w++) sum += s_count[w][threadIdx.x];
    if (sum) atomicAdd(t.words + threadIdx.x, sum);
  }
}

/* ---- read-outs: plain loads, behind the walks on the same stream (occ_lookup, occ_box_key: occupancy_read.h) ----------------- */
__device__ __forceinline__ void occ_write(unsigned long long word, const OccStateRule& sr, unsigned long long i, uint32_t* __restrict__ counts_out,
                                          uint8_t* __restrict__ state_out) {
  const uint32_t hits = (uint32_t)(word >> 32), passes = (uint32_t)word;
  if (counts_out) counts_out[2 * i] = hits, counts_out[2 * i + 1] = passes;
  if (state_out) state_out[i] = (uint8_t)occ_state(hits, passes, sr);
}

__global__ __launch_bounds__(kOccThreads) void occupancy_query_kernel(OccTable t, double leaf, OccStateRule sr, const double* __restrict__ pts,
                                                                      uint32_t stride, unsigned long long n, uint32_t* __restrict__ counts_out,
                                                                      uint8_t* __restrict__ state_out) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kOccThreads + threadIdx.x;
  if (i >= n) return;
  uint64_t key = 0;
  uint32_t u[3];
  const bool ok = cloud_cell(load_point_strided(pts, i, stride), leaf, key, u);
  occ_write(ok ? occ_lookup(t, key) : 0ull, sr, i, counts_out, state_out);
}

__global__ __launch_bounds__(kOccThreads) void occupancy_box_kernel(OccTable t, OccStateRule sr, OccBox box, uint32_t* __restrict__ counts_out,
                                                                    uint8_t* __restrict__ state_out) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kOccThreads + threadIdx.x;
  const unsigned long long plane = (unsigned long long)box.dims[0] * box.dims[1];
  if (i >= plane * box.dims[2]) return;
  const unsigned long long in_plane = i % plane;
  uint64_t key;
  const bool ok = occ_box_key(box, (uint32_t)(in_plane % box.dims[0]), (uint32_t)(in_plane / box.dims[0]), (uint32_t)(i / plane), key);
  occ_write(ok ? occ_lookup(t, key) : 0ull, sr, i, counts_out, state_out);
}

// one column per thread: OCCUPIED if any of its levels is, otherwise FREE if any is, otherwise UNKNOWN
__global__ __launch_bounds__(kOccThreads) void occupancy_slice_kernel(OccTable t, OccStateRule sr, OccBox box, uint8_t* __restrict__ grid_out) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kOccThreads + threadIdx.x;
  if (i >= (unsigned long long)box.dims[0] * box.dims[1]) return;
  const uint32_t x = (uint32_t)(i % box.dims[0]), y = (uint32_t)(i / box.dims[0]);
  uint32_t state = kOccUnknown;
  for (uint32_t z = 0; z < box.dims[2] && state != kOccOccupied; z++) {
    uint64_t key;
    if (!occ_box_key(box, x, y, z, key)) continue;
    const unsigned long long word = occ_lookup(t, key);
    const uint32_t st = occ_state((uint32_t)(word >> 32), (uint32_t)word, sr);
    state = st > state ? st : state;
  }
  grid_out[i] = (uint8_t)state;
}

inline dim3 occ_blocks(unsigned long long n) { return dim3((uint32_t)((n + kOccThreads - 1) / kOccThreads)); }

template <typename T, bool kCombine>
void walk(const void* d_points, uint32_t stride, const OrgOffsets& offs, uint32_t n_clouds, unsigned long long p0, uint32_t n, const double* d_poses,
          const OccRule& rule, const OccTable& t, hipStream_t s) {
  launch_kernel((occupancy_walk_kernel<T, kCombine>), occ_blocks(n), dim3(kOccThreads), 0, s, static_cast<const T*>(d_points), stride, offs, n_clouds, p0, n,
                d_poses, rule, t);
}

}  // namespace

void launch_occupancy_walk(const void* d_points, bool f32, uint32_t stride, const OrgOffsets& offs, uint32_t n_clouds, unsigned long long p0,
                           uint32_t n, const double* d_poses, const OccRule& rule, const OccTable& t, bool combine, hipStream_t s) {
  if (f32) {
    if (combine) walk<float, true>(d_points, stride, offs, n_clouds, p0, n, d_poses, rule, t, s);
    else walk<float, false>(d_points, stride, offs, n_clouds, p0, n, d_poses, rule, t, s);
  } else {
    if (combine) walk<double, true>(d_points, stride, offs, n_clouds, p0, n, d_poses, rule, t, s);
    else walk<double, false>(d_points, stride, offs, n_clouds, p0, n, d_poses, rule, t, s);
  }
}

void launch_occupancy_query(const OccTable& t, double leaf, const OccStateRule& sr, const double* d_points, uint32_t stride, unsigned long long n,
                            uint32_t* d_counts_out, uint8_t* d_state_out, hipStream_t s) {
  launch_kernel(occupancy_query_kernel, occ_blocks(n), dim3(kOccThreads), 0, s, t, leaf, sr, d_points, stride, n, d_counts_out, d_state_out);
}

void launch_occupancy_box(const OccTable& t, const OccStateRule& sr, const OccBox& box, uint32_t* d_counts_out, uint8_t* d_state_out, hipStream_t s) {
  const unsigned long long n = (unsigned long long)box.dims[0] * box.dims[1] * box.dims[2];
  launch_kernel(occupancy_box_kernel, occ_blocks(n), dim3(kOccThreads), 0, s, t, sr, box, d_counts_out, d_state_out);
}

void launch_occupancy_slice(const OccTable& t, const OccStateRule& sr, const OccBox& box, uint8_t* d_grid_out, hipStream_t s) {
  launch_kernel(occupancy_slice_kernel, occ_blocks((unsigned long long)box.dims[0] * box.dims[1]), dim3(kOccThreads), 0, s, t, sr, box, d_grid_out);
}

}  // namespace loamx
