// localize_kernels.hip — scan-to-map localisation on a surfel map (loamx.h, "surfel localisation"; arithmetic: localize_math.h).
// Three kernels. localize_planes_kernel turns every listed voxel into a 64-byte plane record at its slot (and copies the call's
// poses into the per-cloud state); localize_accumulate_kernel evaluates the points of every cloud at its current pose and leaves
// one partial per (cloud, chunk); localize_step_kernel adds a cloud's partials in chunk order and runs the solve of one
// iteration, or writes the records of the call. A call enqueues 1 + groups (2 max_iterations + 2) launches up front and reads
// nothing back. No atomics, no waits between workgroups; the table is read by plain loads behind the kernel boundary of the
// last add (the rule of voxel_find).
#include "loamx_internal.h"
#include "localize_math.h"
#include "surfel_slot.h"
#include "voxel_table.h"

namespace loamx {
namespace {

static_assert(sizeof(LocPlane) == 64 && alignof(LocPlane) == 64, "a plane record is 64 bytes, 64-byte aligned");
static_assert(sizeof(LocPartial::s) == kInfoSums * sizeof(double) && sizeof(LocPartial) == 256, "LocPartial holds the sums of info_math.h");
// Candidates whose first probes are in flight together, and the waves per SIMD the cached form is bounded for. With all seven in
// flight the cached form needs 144 VGPRs (3 waves per SIMD); four at a time fit the 128 of 4 waves without scratch, at the same
// measured time (EXPERIMENTS.md). The plain form is not bounded: surfel_finish beside the 28 sums needs 156.
// (The two macros exist to rebuild the other row of that experiment: -DLOAMX_LOC_IN_FLIGHT=7 -DLOAMX_LOC_WAVES=1. The build never
// sets them.)
#ifndef LOAMX_LOC_IN_FLIGHT
#define LOAMX_LOC_IN_FLIGHT 4
#endif
#ifndef LOAMX_LOC_WAVES
#define LOAMX_LOC_WAVES 4
#endif
constexpr int kLocInFlight = LOAMX_LOC_IN_FLIGHT;
static_assert(kLocCounters <= 8, "LocPartial::c holds the counters");

// one listed voxel per thread: surfel_finish and the usable test, one record at the voxel's SLOT. Thread j < n_clouds also sets
// up the state of cloud j from the call's poses (before any launch writes d_poses_out, which may be the same array).
// A crop of the map (crop_kernels.hip) rebuilds the table, so a voxel may sit in another slot than in the call before, and slots that
// held a removed voxel keep the record an earlier call wrote. That is harmless: the cache is rebuilt here for every listed voxel on
// every call, the accumulate kernel reads a record only at a slot it reached through a key (voxel_find), and every key of a map that
// has not overflowed is listed.
__global__ __launch_bounds__(kLocThreads) void localize_planes_kernel(ListedTable t, double leaf, uint32_t min_points, double planarity,
                                                                      LocPlane* __restrict__ cache, const double* __restrict__ poses_in,
                                                                      uint32_t n_clouds, uint32_t max_iterations, LocState* __restrict__ state) {
  const uint32_t j = blockIdx.x * kLocThreads + threadIdx.x;
  if (j < n_clouds) {
    double P[7];
#pragma unroll
    for (int k = 0; k < 7; k++) P[k] = poses_in[(size_t)j * 7 + k];
    LocState S;
    loc_state_init(S, P, max_iterations);
    state[j] = S;
  }
  // LISTED voxels only: a map that has overflowed (loamx.h: from the first overflow only "every call returns" is promised) holds
  // claimed slots that are not in the list, whose records here stay what they were
  if (!cache || j >= t.max_voxels || j >= t.lens[kCloudLenListed]) return;
  const uint32_t s = t.list[j];  // < 2^log2_cap: the list holds claimed slots only
  cache[s] = loc_plane_of(surfel_of_slot(t, s, t.count[s], leaf), min_points, planarity);
}

// voxel_find from a first probe whose key is already in a register: the same slot sequence, by plain loads
__device__ __forceinline__ uint32_t find_from(const unsigned long long* __restrict__ keys, uint32_t log2_cap, uint64_t key, uint32_t s0,
                                              unsigned long long k0) {
  if (k0 == key) return s0;
  if (k0 == kVoxelEmpty) return kMapNoSlot;
  const uint32_t mask = (uint32_t)((1ull << log2_cap) - 1ull);
  uint32_t s = (s0 + 1u) & mask;
  for (uint32_t probe = 1; probe <= mask; probe++) {
    const unsigned long long k = keys[s];
    if (k == key) return s;
    if (k == kVoxelEmpty) return kMapNoSlot;
    s = (s + 1u) & mask;
  }
  return kMapNoSlot;
}

// a plane record as four 16-byte loads
__device__ __forceinline__ LocPlane load_plane(const LocPlane* __restrict__ cache, uint32_t s) {
  const double2* q = reinterpret_cast<const double2*>(cache + s);
  const double2 a = q[0], b = q[1], c = q[2];
  const uint4 d = reinterpret_cast<const uint4*>(cache + s)[3];
  LocPlane p;
  p.mean[0] = a.x, p.mean[1] = a.y, p.mean[2] = b.x, p.normal[0] = b.y, p.normal[1] = c.x, p.normal[2] = c.y;
  p.count = d.x, p.usable = d.y, p.pad[0] = 0u, p.pad[1] = 0u;
  return p;
}

// the partial of (cloud c, chunk 0) of a launch: clouds back to back, each with room for its own chunks (a cloud of n points has at
// most n / kLocChunk + 1, and floor(a + n) - floor(a) >= floor(n))
__device__ __forceinline__ size_t partial_base(const OrgOffsets& offs, uint32_t c) {
  return (size_t)((offs.off[c] - offs.off[0]) / kLocChunk) + c;
}

/* Grid (chunks of the launch's largest cloud, clouds of the launch). Thread t of chunk k takes the points k kLocChunk + t,
 * + 256, ... of its cloud in that order; then the shuffle tree 32 .. 1, then the four wavefronts in order through LDS: the order
 * of a cloud's sums is a function of the cloud alone. kPlanes: the candidates' records come from the plane cache, and the first
 * probes of kLocInFlight candidates are in flight before any of them is looked at (the kernel waits on gathers, not on bandwidth); otherwise each
 * candidate is found and finished in turn (surfel_of_slot), which gives the same bytes through the same functions. */
template <typename T, bool kPlanes>
__global__ __launch_bounds__(kLocThreads, kPlanes ? LOAMX_LOC_WAVES : 1) void localize_accumulate_kernel(const T* __restrict__ pts, uint32_t stride, OrgOffsets offs,
                                                                          const LocState* __restrict__ state, LocRule R, ListedTable t,
                                                                          const LocPlane* __restrict__ cache, uint32_t final_pass,
                                                                          LocPartial* __restrict__ partials) {
  __shared__ double s_sum[kLocThreads / 64][kInfoSums];
  __shared__ uint32_t s_cnt[kLocThreads / 64][kLocCounters];
  const uint32_t c = blockIdx.y, chunk = blockIdx.x;
  const unsigned long long b0 = offs.off[c], n = offs.off[c + 1] - b0, base = (unsigned long long)chunk * kLocChunk;
  if (base >= n) return;  // (uniform) beyond the cloud's chunks
  const LocState* S = state + c;
  if (!final_pass && S->done) return;  // (uniform) the cloud has stopped
  double P[7];  // (uniform loads: scalar registers)
#pragma unroll
  for (int k = 0; k < 7; k++) P[k] = S->pose[k];
  const int nk = R.neighborhood == 7u ? kLocCandidates : 1;
  LocAcc acc;
  loc_acc_clear(acc);
#pragma unroll 1
  for (int it = 0; it < kLocItems; it++) {
    const unsigned long long i = base + (unsigned long long)it * kLocThreads + threadIdx.x;
    if (i >= n) break;
    const Vec3 p = load_point_strided(pts, b0 + i, stride);
    Vec3 v = v3(0.0, 0.0, 0.0);
    uint64_t home = 0;
    const bool moved = loc_move(R, P, p, v, home);
    int best = -1;
    double best_d2 = 0.0;
    LocPlane best_plane = {};
    if (!moved) {
      // (no candidates)
    } else if (kPlanes) {
      // kLocInFlight candidates at a time: their first probes are issued together, before any key is looked at
#pragma unroll
      for (int g = 0; g < kLocCandidates; g += kLocInFlight) {
        uint64_t key[kLocInFlight];
        uint32_t slot[kLocInFlight];
        unsigned long long k0[kLocInFlight];
        bool has[kLocInFlight];
#pragma unroll
        for (int j = 0; j < kLocInFlight; j++) {
          const int k = g + j;
          key[j] = home;  // (a lane of the group beyond the candidates hashes the home key and loads nothing)
          has[j] = k < nk && loc_candidate_key(home, k < kLocCandidates ? k : 0, key[j]);
          slot[j] = voxel_hash(key[j], t.log2_cap);  // < 2^log2_cap for any key
          k0[j] = has[j] ? t.keys[slot[j]] : (unsigned long long)kVoxelEmpty;
        }
#pragma unroll
        for (int j = 0; j < kLocInFlight; j++) {
          const uint32_t s = has[j] ? find_from(t.keys, t.log2_cap, key[j], slot[j], k0[j]) : kMapNoSlot;
          if (s != kMapNoSlot) loc_offer(v, load_plane(cache, s), g + j, best_d2, best, best_plane);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
#pragma unroll 1
      for (int k = 0; k < nk; k++) {
        uint64_t key;
        if (!loc_candidate_key(home, k, key)) continue;
        const uint32_t s = voxel_find(t.keys, t.log2_cap, key);
        if (s == kMapNoSlot) continue;
        loc_offer(v, loc_plane_of(surfel_of_slot(t, s, t.count[s], R.leaf), R.min_points, R.planarity), k, best_d2, best, best_plane);
      }
    }
    // the sums are touched in ONE place, whatever became of the point
    acc.c[kLocUnused] += moved ? 0u : 1u;
    acc.c[kLocNoSurfel] += moved && best < 0 ? 1u : 0u;
    loc_accumulate(R, v, best_plane, best >= 0, acc);
  }
  // wavefront shuffle reduction, then LDS across the 4 wavefronts, fixed order => deterministic
#pragma unroll
  for (int j = 0; j < kInfoSums; j++) {
    double x = acc.s[j];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_down(x, off);
    acc.s[j] = x;
  }
#pragma unroll
  for (int j = 0; j < kLocCounters; j++) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc.c[j] += __shfl_down(acc.c[j], off);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < kInfoSums; j++) s_sum[wave][j] = acc.s[j];
#pragma unroll
    for (int j = 0; j < kLocCounters; j++) s_cnt[wave][j] = acc.c[j];
  }
  __syncthreads();
  LocPartial& out = partials[partial_base(offs, c) + chunk];
  if (threadIdx.x < kInfoSums) {
    double x = s_sum[0][threadIdx.x];
    for (int w = 1; w < kLocThreads / 64; w++) x += s_sum[w][threadIdx.x];
    out.s[threadIdx.x] = x;
  } else if (threadIdx.x < kInfoSums + kLocCounters) {
    const int j = threadIdx.x - kInfoSums;
    uint32_t x = s_cnt[0][j];
    for (int w = 1; w < kLocThreads / 64; w++) x += s_cnt[w][j];
    out.c[j] = x;
  }
}

// one cloud per thread: its partials in chunk order, then one iteration of the solve (or, in the final pass, the records)
__global__ __launch_bounds__(64) void localize_step_kernel(OrgOffsets offs, uint32_t n_clouds, LocState* __restrict__ state, LocSolve P,
                                                           const LocPartial* __restrict__ partials, uint32_t final_pass,
                                                           double* __restrict__ poses_out, LocResult* __restrict__ results,
                                                           loamx_reg_information* __restrict__ info) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_clouds) return;
  LocState S = state[c];
  if (!final_pass && S.done) return;
  const unsigned long long n = offs.off[c + 1] - offs.off[c];
  const uint32_t chunks = (uint32_t)((n + kLocChunk - 1) / kLocChunk);
  const LocPartial* part = partials + partial_base(offs, c);
  double s[kInfoSums];
  uint32_t cnt[kLocCounters];
#pragma unroll
  for (int j = 0; j < kInfoSums; j++) s[j] = 0.0;
#pragma unroll
  for (int j = 0; j < kLocCounters; j++) cnt[j] = 0u;
  for (uint32_t b = 0; b < chunks; b++) {  // chunk order
#pragma unroll
    for (int j = 0; j < kInfoSums; j++) s[j] += part[b].s[j];
#pragma unroll
    for (int j = 0; j < kLocCounters; j++) cnt[j] += part[b].c[j];
  }
  if (!final_pass) {
    loc_iterate(S, P, s, cnt[kLocRows]);
    state[c] = S;
    return;
  }
  LocResult out;
  loamx_reg_information rec;
  loc_finish(S, P, s, cnt, out, info ? &rec : nullptr);
  results[c] = out;
  if (info) info[c] = rec;
#pragma unroll
  for (int k = 0; k < 7; k++) poses_out[(size_t)c * 7 + k] = S.pose[k];
}

template <typename T, bool kPlanes>
void accumulate(const void* d_points, uint32_t stride, const OrgOffsets& offs, uint32_t n_clouds, uint32_t chunks, const LocState* state,
                const LocRule& rule, const ListedTable& t, const LocPlane* cache, bool final_pass, LocPartial* partials, hipStream_t s) {
  launch_kernel((localize_accumulate_kernel<T, kPlanes>), dim3(chunks, n_clouds), dim3(kLocThreads), 0, s, static_cast<const T*>(d_points), stride,
                offs, state, rule, t, cache, final_pass ? 1u : 0u, partials);
}

}  // namespace

size_t localize_partials(size_t max_points) { return max_points / kLocChunk + kOrgChunkClouds + 1; }

void launch_localize_planes(const ListedTable& t, double leaf, uint32_t min_points, double planarity, LocPlane* cache, const double* d_poses_in,
                            uint32_t n_clouds, uint32_t max_iterations, LocState* state, hipStream_t s) {
  const uint32_t most = cache && t.max_voxels > n_clouds ? t.max_voxels : n_clouds;
  if (most == 0) return;
  launch_kernel(localize_planes_kernel, dim3((most + kLocThreads - 1) / kLocThreads), dim3(kLocThreads), 0, s, t, leaf, min_points, planarity, cache,
                d_poses_in, n_clouds, max_iterations, state);
}

void launch_localize_accumulate(const void* d_points, bool f32, uint32_t stride, const OrgOffsets& offs, uint32_t n_clouds, unsigned long long largest,
                                const LocState* state, const LocRule& rule, const ListedTable& t, const LocPlane* cache, bool final_pass,
                                LocPartial* partials, hipStream_t s) {
  const uint32_t chunks = (uint32_t)((largest + kLocChunk - 1) / kLocChunk);
  if (n_clouds == 0 || chunks == 0) return;
  if (f32) {
    if (cache) accumulate<float, true>(d_points, stride, offs, n_clouds, chunks, state, rule, t, cache, final_pass, partials, s);
    else accumulate<float, false>(d_points, stride, offs, n_clouds, chunks, state, rule, t, cache, final_pass, partials, s);
  } else {
    if (cache) accumulate<double, true>(d_points, stride, offs, n_clouds, chunks, state, rule, t, cache, final_pass, partials, s);
    else accumulate<double, false>(d_points, stride, offs, n_clouds, chunks, state, rule, t, cache, final_pass, partials, s);
  }
}

void launch_localize_step(const OrgOffsets& offs, uint32_t n_clouds, LocState* state, const LocSolve& P, const LocPartial* partials, bool final_pass,
                          double* d_poses_out, LocResult* d_results, loamx_reg_information* d_info, hipStream_t s) {
  if (n_clouds == 0) return;
  launch_kernel(localize_step_kernel, dim3((n_clouds + 63) / 64), dim3(64), 0, s, offs, n_clouds, state, P, partials, final_pass ? 1u : 0u, d_poses_out,
                d_results, d_info);
}

}  // namespace loamx
