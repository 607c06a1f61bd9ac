// surfel_kernels.hip — the surfel map (loamx.h, "surfel map"): posed clouds accumulated on a voxel grid as integer first and second
// moments plus an integer view sum, the voxel list in order of first appearance, and the records (mean, covariance, eigenvalues,
// oriented normal) read out in that order or looked up per point. Per-point arithmetic and the finish: surfel_math.h; the table:
// voxel_table.h; the stable compaction: map_compact.h.
//
// What this unit adds to the listed voxel table it shares with the cloud map: its payload for the accumulate kernel
// (listed_accumulate.h), the scatter of its emit (behind the flags of listed_kernels.hip, where the launches of an add and of an
// emit are counted out) and the query.
#include "listed_accumulate.h"
#include "map_compact.h"
#include "surfel_math.h"
#include "surfel_slot.h"

namespace loamx {
namespace {

static_assert(kSurfelSlotWords == (uint32_t)kSurfelMoments, "a slot holds the twelve words of surfel_point");
static_assert(sizeof(loamx_surfel) == 128, "loamx_surfel is 128 bytes");

// a slot holds the twelve words of surfel_point. A head issues one CAS chain, twelve 64-bit atomicAdd, one 32-bit add and one
// atomicMin: 14 atomics against the cloud map's 5, which is what run combining saves per combined lane. The view terms are signed
// and travel as two's-complement words; |W| < 2^62 by the clamp.
struct SurfelPayload {
  static constexpr int kWords = kSurfelMoments;
  static __device__ __forceinline__ void point(const uint32_t u[3], Vec3 o, Vec3 p, double leaf, unsigned long long m[kWords]) {
    surfel_point(u, o, p, leaf, m);
  }
};

/* ---- read-outs (the record of a slot: surfel_of_slot of surfel_slot.h) ------------------------------------------------------- */
// one listed voxel per thread, surfel_finish in registers, one 128-byte record out (and the mean and the normal on their own)
__global__ __launch_bounds__(kListedThreads) void surfel_emit_scatter_kernel(const uint8_t* __restrict__ keep, const uint32_t* __restrict__ tiles,
                                                                             ListedTable t, double leaf, unsigned long long capacity,
                                                                             loamx_surfel* __restrict__ out, double* __restrict__ xyz_out,
                                                                             double* __restrict__ normal_out) {
  __shared__ uint32_t s_wave[4];
  const uint32_t j = blockIdx.x * kListedThreads + threadIdx.x;
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
__global__ __launch_bounds__(kListedThreads) void surfel_query_kernel(ListedTable t, double leaf, uint32_t min_points, const double* __restrict__ pts,
                                                                      uint32_t stride, unsigned long long n, loamx_surfel* __restrict__ out,
                                                                      double* __restrict__ distance_out, uint32_t* __restrict__ count_out) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kListedThreads + threadIdx.x;
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

}  // namespace

void launch_surfel_accumulate(const void* d_points, bool f32, uint32_t stride, const OrgOffsets& offs, uint32_t n_clouds, unsigned long long p0,
                              uint32_t n, uint32_t g0, const double* d_poses, const CloudRule& rule, const ListedTable& t, bool combine, uint32_t* d_slot,
                              hipStream_t s) {
  launch_listed_accumulate<SurfelPayload>(d_points, f32, stride, offs, n_clouds, p0, n, g0, d_poses, rule, t, combine, d_slot, s);
}

void launch_surfel_emit(const ListedTable& t, double leaf, uint32_t min_points, uint8_t* d_keep, uint32_t* d_tiles, loamx_surfel* d_out,
                        double* d_xyz_out, double* d_normal_out, size_t capacity, uint32_t* d_n_out, hipStream_t s) {
  launch_listed_emit_flags(t, min_points, d_keep, d_tiles, d_n_out, s);
  if (capacity == 0 || (!d_out && !d_xyz_out && !d_normal_out)) return;  // (only the number was asked for)
  launch_kernel(surfel_emit_scatter_kernel, listed_tiles(t.max_voxels), dim3(kListedThreads), 0, s, (const uint8_t*)d_keep, (const uint32_t*)d_tiles, t,
                leaf, (unsigned long long)capacity, d_out, d_xyz_out, d_normal_out);
}

void launch_surfel_query(const ListedTable& t, double leaf, uint32_t min_points, const double* d_points, uint32_t stride, unsigned long long n,
                         loamx_surfel* d_out, double* d_distance_out, uint32_t* d_count_out, hipStream_t s) {
  if (n == 0 || (!d_out && !d_distance_out && !d_count_out)) return;
  launch_kernel(surfel_query_kernel, listed_tiles(n), dim3(kListedThreads), 0, s, t, leaf, min_points, d_points, stride, n, d_out, d_distance_out,
                d_count_out);
}

}  // namespace loamx
