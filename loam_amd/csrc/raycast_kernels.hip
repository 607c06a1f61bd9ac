// raycast_kernels.hip — the occupancy ray cast (loamx.h, "occupancy ray casting"): segments, or the beams of scans rendered at
// poses, walked through the occupancy map's table until the first voxel that stops them. Per-ray arithmetic: raycast_math.h. The
// table is only read (occ_lookup: plain loads, behind a kernel boundary from the last claim), a ray depends on that ray alone and
// the counters are integer sums: every schedule and both forms leave the same bytes. No launch waits for another workgroup, and a
// lane takes at most max_steps + 1 trips of the loop.
#include "loamx_internal.h"
#include "occupancy_read.h"
#include "raycast_math.h"
#include "voxel_table.h"

namespace loamx {
namespace {

constexpr int kRayThreads = 256;

/* The count words of one trip: `on` lanes want the word of `key`.
 *
 * kCombine: the lanes of a wavefront are neighbouring rays or beams, and near their origin they stand in the same voxel trip after
 * trip. Lanes that are `on` and hold the same key in adjacent lanes form a run (run_head, voxel_table.h: A B A is three runs, and a
 * lane that is not `on` ends a run); the head of a run alone looks the key up and the others take the word from it by shuffle. A
 * lane that is no head has the lane before it in its run, so its head is the nearest head at or below it. `probes` counts the
 * look-ups; it is wave-uniform. */
template <bool kCombine>
__device__ __forceinline__ unsigned long long ray_words(bool on, uint64_t key, uint32_t lane, const OccTable& t, uint32_t& probes) {
  const unsigned long long m_on = __ballot(on);
  if (m_on == 0ull) return 0ull;  // (uniform)
  unsigned long long word = 0ull;
  if (kCombine) {
    const bool head = run_head(on, key, lane, m_on);
    const unsigned long long m_head = __ballot(head);
    probes += (uint32_t)__popcll(m_head);
    if (head) word = occ_lookup(t, key);
    const unsigned long long below = m_head & (~0ull >> (63u - lane));  // (an `on` lane has a head at or below it)
    const int src = on ? 63 - __builtin_clzll(below | 1ull) : (int)lane;
    const uint32_t lo = __shfl((uint32_t)word, src, 64), hi = __shfl((uint32_t)(word >> 32), src, 64);
    word = (unsigned long long)hi << 32 | lo;
  } else {
    probes += (uint32_t)__popcll(m_on);
    if (on) word = occ_lookup(t, key);
  }
  return word;
}

struct RayCall {
  // cast: segment i from origins + i stride to ends + i stride
  const double* origins;
  const double* ends;
  uint32_t stride;
  // render: ray i is beam i % n_beams of pose i / n_beams
  const double* dirs;
  const double* poses;
  uint32_t n_beams;
  double max_range;
  unsigned long long n;
  RayRule rule;
  double leaf;
  OccStateRule sr;
  RayRecord* records;  // [n], or nullptr (render only)
  double* scans;       // [n][3], or nullptr
  double* ranges;      // [n], or nullptr
  unsigned long long* census;  // [kRayCensusWords]: added to
};

/* Thread i holds ray i. The wavefront loops while any lane is live; in each trip the live lanes that test their voxel take its count
 * word through ray_words and every live lane makes its visit (ray_visit: stop, or step on). Counters: ballots summed per wavefront
 * in uniform registers, met in LDS, one atomic per workgroup and word that has something to add. */
template <bool kCombine, bool kRender>
__global__ __launch_bounds__(kRayThreads) void raycast_kernel(RayCall c, OccTable t) {
  __shared__ uint32_t s_count[kRayThreads / 64][kRayCensusWords];
  const unsigned long long i = (unsigned long long)blockIdx.x * kRayThreads + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  const bool mine = i < c.n;

  RayCast r;
  ray_idle(r, kRayClear);
  Vec3 d = v3(0.0, 0.0, 0.0);
  if (mine) {
    Vec3 o, e;
    bool ok = true;
    if (kRender) {
      const unsigned long long pose = i / c.n_beams, beam = i % c.n_beams;
      double P[7];
#pragma unroll
      for (int k = 0; k < 7; k++) P[k] = c.poses[pose * 7 + k];
      d = v3(c.dirs[beam * 3], c.dirs[beam * 3 + 1], c.dirs[beam * 3 + 2]);
      ok = ray_beam(P, d, c.max_range, o, e);
    } else {
      o = load_point_strided(c.origins, i, c.stride), e = load_point_strided(c.ends, i, c.stride);
    }
    if (ok) ray_begin(o, e, c.leaf, c.rule, r);
    else ray_idle(r, kRayInvalid);
  }

  uint32_t n_tested = 0, n_probes = 0;
  while (__ballot(r.live) != 0ull) {
    const bool tests = ray_tests(r, c.rule);
    n_tested += (uint32_t)__popcll(__ballot(tests));
    const unsigned long long word = ray_words<kCombine>(tests, occ_walk_key(r.w), lane, t, n_probes);
    if (r.live) ray_visit(r, word, c.sr, c.rule);
  }

  RayRecord rec;
  ray_record(r, rec);
  if (mine) {
    if (c.records) c.records[i] = rec;
    if (kRender) {
      double range;
      Vec3 p;
      ray_return(rec, d, c.max_range, c.rule.hit_at, range, p);
      if (c.ranges) c.ranges[i] = range;
      if (c.scans) c.scans[3 * i] = p.x, c.scans[3 * i + 1] = p.y, c.scans[3 * i + 2] = p.z;
    }
  }

  uint32_t by_status[kRayStatuses];
#pragma unroll
  for (int s = 0; s < kRayStatuses; s++) by_status[s] = (uint32_t)__popcll(__ballot(mine && r.status == (uint32_t)s));
  if (lane == 0) {
    uint32_t* w = s_count[threadIdx.x >> 6];
    w[kRayWordVisits] = n_tested, w[kRayWordProbes] = n_probes;
#pragma unroll
    for (int s = 0; s < kRayStatuses; s++) w[kRayWordStatus + s] = by_status[s];
  }
  __syncthreads();
  if (threadIdx.x < kRayCensusWords) {
    unsigned long long sum = 0;
    for (int w = 0; w < kRayThreads / 64; w++) sum += s_count[w][threadIdx.x];
    if (sum) atomicAdd(c.census + threadIdx.x, sum);
  }
}

template <bool kCombine, bool kRender>
void cast(const RayCall& c, const OccTable& t, hipStream_t s) {
  launch_kernel((raycast_kernel<kCombine, kRender>), dim3((uint32_t)((c.n + kRayThreads - 1) / kRayThreads)), dim3(kRayThreads), 0, s, c, t);
}

void launch(const RayCall& c, const OccTable& t, bool combine, bool render, hipStream_t s) {
  if (render) {
    if (combine) cast<true, true>(c, t, s);
    else cast<false, true>(c, t, s);
  } else {
    if (combine) cast<true, false>(c, t, s);
    else cast<false, false>(c, t, s);
  }
}

}  // namespace

static_assert(sizeof(RayRecord) == 40 && sizeof(RayRecord) == sizeof(loamx_ray_record), "a ray record is 40 bytes");

void launch_raycast(const OccTable& t, double leaf, const OccStateRule& sr, const RayRule& rule, const double* d_origins, const double* d_ends,
                    uint32_t stride, unsigned long long n, RayRecord* d_records, unsigned long long* d_census, bool combine, hipStream_t s) {
  RayCall c = {};
  c.origins = d_origins, c.ends = d_ends, c.stride = stride, c.n = n, c.rule = rule, c.leaf = leaf, c.sr = sr;
  c.records = d_records, c.census = d_census;
  launch(c, t, combine, false, s);
}

void launch_raycast_render(const OccTable& t, double leaf, const OccStateRule& sr, const RayRule& rule, const double* d_dirs, uint32_t n_beams,
                           const double* d_poses, unsigned long long n_poses, double max_range, double* d_scans, double* d_ranges,
                           RayRecord* d_records, unsigned long long* d_census, bool combine, hipStream_t s) {
  RayCall c = {};
  c.dirs = d_dirs, c.poses = d_poses, c.n_beams = n_beams, c.max_range = max_range, c.n = n_poses * n_beams, c.rule = rule, c.leaf = leaf, c.sr = sr;
  c.records = d_records, c.scans = d_scans, c.ranges = d_ranges, c.census = d_census;
  launch(c, t, combine, true, s);
}

}  // namespace loamx
