// visibility_kernels.hip — map cleaning (loamx.h, "map cleaning"): the visibility votes of map points over posed scans, and the
// decision over the votes with the ordered compaction of the points that stay. Per-pair arithmetic: visibility_math.h; the
// stable compaction is the one of map_kernels.hip (map_compact.h).
//
// The votes are integer counts: every split of the scans over workgroups and both forms of the kernel give the same bytes.
// No launch waits for another workgroup, no loop has a bound that depends on the data beyond the bisections of organize_math.h.
#include "loamx_internal.h"
#include "map_compact.h"
#include "visibility_math.h"

namespace loamx {
namespace {

constexpr int kVisThreads = (int)kMapTile;  // one map point per thread; the tiles of the compaction are the workgroups

/* ---- ranges -----------------------------------------------------------------------------------------------------------------
 * One thread per cell of every scan: its squared range, -1 where the cell is not usable. */
template <typename T>
__global__ __launch_bounds__(kVisThreads) void visibility_ranges_kernel(const T* __restrict__ scans, unsigned long long n_cells, double min2,
                                                                        double* __restrict__ ranges) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kVisThreads + threadIdx.x;
  if (i >= n_cells) return;
  const T* q = scans + i * 3;
  ranges[i] = vis_cell_r2((double)q[0], (double)q[1], (double)q[2], min2);
}

/* ---- votes ----------------------------------------------------------------------------------------------------------------
 * Thread i holds map point blockIdx.x * 256 + i, workgroup row blockIdx.y holds the scans [y chunk, (y + 1) chunk). The scan's
 * pose and base pointer are the same for the whole workgroup (scalar loads, scalar address arithmetic). kLds: the two layout
 * tables are staged in LDS once per workgroup (col_dirs W x 16 B, then line_tans (H + 1) x 8 B) and the bisections read them
 * there; otherwise (tables beyond kVisLdsTableBytes) they are read where the layout keeps them. The range test comes first:
 * on a long drive most pairs fail it, and neighbouring threads hold neighbouring voxels, so whole wavefronts skip a scan.
 * kRanges: the window reads the 8-byte squared ranges visibility_ranges_kernel left, not the scans' points.
 *
 * The four counts are kept in registers over the chunk. kAtomic == false (one chunk, no accumulation): one 16-byte store per
 * point; otherwise one integer atomicAdd per non-zero field (the caller has zeroed the votes of a call that does not
 * accumulate). The two census words: ballots meet in LDS, one 64-bit atomic per workgroup and word that has something to add. */
template <typename T, bool kLds, bool kRanges, bool kAtomic>
__global__ __launch_bounds__(kVisThreads) void visibility_votes_kernel(const double* __restrict__ points, uint32_t stride, uint32_t n_points,
                                                                       const T* __restrict__ scans, const double* __restrict__ ranges,
                                                                       uint32_t n_scans, uint32_t chunk, const double* __restrict__ poses,
                                                                       OrgTables tab, VisRule rule, loamx_visibility_tally* __restrict__ votes,
                                                                       unsigned long long* __restrict__ census) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ uint32_t s_count[4][2];
  OrgTables t = tab;
  if (kLds) {
    double* s_dirs = reinterpret_cast<double*>(smem);
    double* s_tans = s_dirs + 2 * (size_t)tab.W;
    for (uint32_t k = threadIdx.x; k < 2 * tab.W; k += kVisThreads) s_dirs[k] = tab.col_dirs[k];
    for (uint32_t k = threadIdx.x; k <= tab.H; k += kVisThreads) s_tans[k] = tab.line_tans[k];
    __syncthreads();
    t.col_dirs = s_dirs, t.line_tans = s_tans;
  }
  t.ring_map = nullptr, t.n_ring_map = 0;

  const uint32_t i = blockIdx.x * kVisThreads + threadIdx.x;
  const bool in = i < n_points;
  Vec3 m = v3(0.0, 0.0, 0.0);
  if (in) {
    const double* p = points + (size_t)i * stride;
    m = v3(p[0], p[1], p[2]);
  }
  const uint32_t s0 = blockIdx.y * chunk, s1 = n_scans - s0 < chunk ? n_scans : s0 + chunk;
  const size_t HW = (size_t)t.H * t.W;
  uint32_t cnt[4] = {0u, 0u, 0u, 0u};
  uint32_t n_in_range = 0, n_projected = 0;
  for (uint32_t s = s0; s < s1; s++) {
    double P[7];
    for (int k = 0; k < 7; k++) P[k] = poses[(size_t)s * 7 + k];
    if (!in) continue;
    const Vec3 p = vis_to_sensor(P, m);
    uint32_t cell;
    double r2;
    const int place = vis_place(t, p, rule, cell, r2);
    if (place == kVisPlaceNone) continue;
    n_in_range++;
    if (place != kVisPlaceProjected) continue;
    n_projected++;
    double lo2, hi2;
    vis_bounds(r2, rule, lo2, hi2);
    int verdict;
    if (kRanges) {
      const double* rs = ranges + (size_t)s * HW;
      verdict = vis_window(cell / t.W, cell % t.W, t.H, t.W, rule, lo2, hi2, [rs](uint32_t c) { return rs[c]; });
    } else {
      const T* scan = scans + (size_t)s * HW * 3;
      const double min2 = rule.min2;
      verdict = vis_window(cell / t.W, cell % t.W, t.H, t.W, rule, lo2, hi2, [scan, min2](uint32_t c) {
        const T* q = scan + (size_t)c * 3;
        return vis_cell_r2((double)q[0], (double)q[1], (double)q[2], min2);
      });
    }
    cnt[0] += verdict == kVisThrough, cnt[1] += verdict == kVisAgree;
    cnt[2] += verdict == kVisOccluded, cnt[3] += verdict == kVisEmpty;
  }

  if (in) {
    if (kAtomic) {
      uint32_t* v = reinterpret_cast<uint32_t*>(votes + i);
      for (int k = 0; k < 4; k++)
        if (cnt[k]) atomicAdd(v + k, cnt[k]);
    } else {
      loamx_visibility_tally v;
      v.through = cnt[0], v.agree = cnt[1], v.occluded = cnt[2], v.empty = cnt[3];
      votes[i] = v;
    }
  }

  // census: wavefront sums by a shuffle tree, the four wavefronts meet in LDS
  for (uint32_t d = 32; d > 0; d >>= 1) {
    n_in_range += __shfl_down(n_in_range, d, 64);
    n_projected += __shfl_down(n_projected, d, 64);
  }
  if ((threadIdx.x & 63u) == 0) s_count[threadIdx.x >> 6][0] = n_in_range, s_count[threadIdx.x >> 6][1] = n_projected;
  __syncthreads();
  if (threadIdx.x < 2) {
    const uint32_t k = threadIdx.x;
    const unsigned long long sum = (unsigned long long)s_count[0][k] + s_count[1][k] + s_count[2][k] + s_count[3][k];
    if (sum) atomicAdd(census + k, sum);
  }
}

/* ---- decide and compact ----------------------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(kVisThreads) void visibility_decide_kernel(const loamx_visibility_tally* __restrict__ votes, uint32_t n,
                                                                        uint32_t min_through, double through_ratio, uint8_t* __restrict__ keep,
                                                                        uint8_t* __restrict__ dynamic_out) {
  const uint32_t i = blockIdx.x * kVisThreads + threadIdx.x;
  if (i >= n) return;
  const loamx_visibility_tally v = votes[i];
  const bool dyn = vis_dynamic(v.through, v.agree, min_through, through_ratio);
  keep[i] = dyn ? 0 : 1;
  if (dynamic_out) dynamic_out[i] = dyn ? 1 : 0;
}

// the kept points behind each other in input order; what does not fit `capacity` is not written
__global__ __launch_bounds__(kVisThreads) void visibility_scatter_kernel(const uint8_t* __restrict__ keep, const uint32_t* __restrict__ tiles, uint32_t n,
                                                                         const double* __restrict__ points, uint32_t stride,
                                                                         unsigned long long capacity, double* __restrict__ xyz_out,
                                                                         uint32_t* __restrict__ index_out) {
  __shared__ uint32_t s_wave[4];
  const uint32_t i = blockIdx.x * kVisThreads + threadIdx.x;
  const bool flag = i < n && keep[i] != 0;
  uint32_t total;
  const uint32_t rank = block_rank(flag, s_wave, total);
  if (!flag) return;
  const uint32_t dst = tiles[blockIdx.x] + rank;
  if (dst >= capacity) return;
  if (xyz_out) {
    const double* p = points + (size_t)i * stride;
    for (int a = 0; a < 3; a++) xyz_out[(size_t)dst * 3 + a] = p[a];
  }
  if (index_out) index_out[dst] = i;
}

inline dim3 vis_tiles(unsigned long long n) { return dim3((uint32_t)((n + kMapTile - 1) / kMapTile)); }

template <typename T, bool kLds, bool kRanges>
void votes_launch(const VisVotesCall& c, hipStream_t s) {
  const dim3 grid(vis_tiles(c.n_points).x, (c.n_scans + c.chunk - 1) / c.chunk);
  const size_t lds = kLds ? vis_table_bytes(c.tab.H, c.tab.W) : 0;
  const T* scans = static_cast<const T*>(c.d_scans);
  if (c.atomic)
    launch_kernel((visibility_votes_kernel<T, kLds, kRanges, true>), grid, dim3(kVisThreads), lds, s, c.d_points, c.stride, c.n_points, scans, c.d_ranges,
                  c.n_scans, c.chunk, c.d_poses, c.tab, c.rule, c.d_votes, c.d_census);
  else
    launch_kernel((visibility_votes_kernel<T, kLds, kRanges, false>), grid, dim3(kVisThreads), lds, s, c.d_points, c.stride, c.n_points, scans, c.d_ranges,
                  c.n_scans, c.chunk, c.d_poses, c.tab, c.rule, c.d_votes, c.d_census);
}

template <typename T>
void votes_launch_t(const VisVotesCall& c, hipStream_t s) {
  const bool lds = vis_table_bytes(c.tab.H, c.tab.W) <= kVisLdsTableBytes;
  if (c.d_ranges) {
    if (lds) votes_launch<T, true, true>(c, s);
    else votes_launch<T, false, true>(c, s);
  } else {
    if (lds) votes_launch<T, true, false>(c, s);
    else votes_launch<T, false, false>(c, s);
  }
}

}  // namespace

// d_ranges: n_scans x H W doubles
void launch_visibility_ranges(const void* d_scans, bool f32, unsigned long long n_cells, double min2, double* d_ranges, hipStream_t s) {
  if (f32) launch_kernel(visibility_ranges_kernel<float>, vis_tiles(n_cells), dim3(kVisThreads), 0, s, static_cast<const float*>(d_scans), n_cells, min2, d_ranges);
  else launch_kernel(visibility_ranges_kernel<double>, vis_tiles(n_cells), dim3(kVisThreads), 0, s, static_cast<const double*>(d_scans), n_cells, min2, d_ranges);
}

// n_points > 0, n_scans > 0, ceil(n_scans / chunk) <= 65535
void launch_visibility_votes(const VisVotesCall& c, hipStream_t s) {
  if (c.f32) votes_launch_t<float>(c, s);
  else votes_launch_t<double>(c, s);
}

// d_keep: n bytes; d_tiles: map_compact_ws_bytes(n). Writes *d_n_out in every case.
void launch_visibility_filter(const loamx_visibility_tally* d_votes, uint32_t n, uint32_t min_through, double through_ratio, const double* d_points,
                              uint32_t stride, uint8_t* d_keep, uint32_t* d_tiles, uint8_t* d_dynamic_out, double* d_xyz_out, uint32_t* d_index_out,
                              size_t capacity, uint32_t* d_n_out, hipStream_t s) {
  if (n) launch_kernel(visibility_decide_kernel, vis_tiles(n), dim3(kVisThreads), 0, s, d_votes, n, min_through, through_ratio, d_keep, d_dynamic_out);
  launch_tile_offsets(d_keep, n, d_tiles, d_n_out, s);
  if (n && capacity && (d_xyz_out || d_index_out))
    launch_kernel(visibility_scatter_kernel, vis_tiles(n), dim3(kVisThreads), 0, s, (const uint8_t*)d_keep, (const uint32_t*)d_tiles, n, d_points, stride,
                  (unsigned long long)capacity, d_xyz_out, d_index_out);
}

}  // namespace loamx
