// distance_kernels.hip — the occupancy distance field (loamx.h, "occupancy distance field"): the exact squared Euclidean distance
// from every voxel of a box (or column of a slice) to the nearest obstacle voxel of the map, capped at R voxels, with the offset to
// that obstacle and the distance in metres. The rule: distance_math.h. Four launches for a box (mask, x, y, z), three for a slice
// (mask, x, y); only the mask launch reads the map's table. Everything is integer and each output element is one thread's own
// minimum: every schedule leaves the same bytes. No atomics, no LDS, nothing read back, no workgroup waits for another, and every
// loop has a bound known before it starts (the probe of the lookup, R / 64 + 2 words, R rows).
#include "distance_math.h"
#include "loamx_internal.h"
#include "occupancy_read.h"

namespace loamx {
namespace {

constexpr int kDistThreads = 256;
constexpr unsigned long long kDistMaskWavesPerLaunch = 1ull << 24;  // 2^30 threads

/* ---- mask -------------------------------------------------------------------------------------------------------------------
 * One voxel of the extended box (kSlice: one column) per lane, x fastest, a wavefront per mask word: word g holds the positions
 * 64 (g % W) .. + 63 of row g / W, positions behind the row's end are 0. The wavefront's ballot is the word; lane 0 stores it. */
template <bool kSlice>
__global__ __launch_bounds__(kDistThreads) void distance_mask_kernel(OccTable t, OccStateRule sr, DistGeom g, unsigned long long wave0,
                                                                     unsigned long long n_waves, unsigned long long* __restrict__ mask) {
  const unsigned long long wave = wave0 + (unsigned long long)blockIdx.x * (kDistThreads / 64) + (threadIdx.x >> 6);
  if (wave >= n_waves) return;  // (uniform in the wavefront)
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long row = wave / g.W;
  const uint32_t xe = (uint32_t)(wave % g.W) * 64u + lane;
  const uint32_t ye = (uint32_t)(row % g.e[1]), ze = (uint32_t)(row / g.e[1]);
  bool obstacle = false;
  if (xe < g.e[0]) {
    const long long vx = (long long)g.vmin[0] - g.R + xe, vy = (long long)g.vmin[1] - g.R + ye;
    uint32_t state = kOccUnknown;
    if (kSlice) {  // the column's state as occupancy_slice_kernel forms it
      for (uint32_t z = 0; z < g.levels && state != kOccOccupied; z++) {
        uint64_t key;
        if (!occ_voxel_key(vx, vy, (long long)g.vmin[2] + z, key)) continue;
        const unsigned long long word = occ_lookup(t, key);
        const uint32_t st = occ_state((uint32_t)(word >> 32), (uint32_t)word, sr);
        state = st > state ? st : state;
      }
    } else {  // the voxel's state as occupancy_box_kernel writes it
      uint64_t key;
      const bool ok = occ_voxel_key(vx, vy, (long long)g.vmin[2] - g.R + ze, key);
      const unsigned long long word = ok ? occ_lookup(t, key) : 0ull;
      state = occ_state((uint32_t)(word >> 32), (uint32_t)word, sr);
    }
    obstacle = dist_obstacle(state, g.unknown_is_obstacle != 0u);
  }
  const unsigned long long word = __ballot(obstacle);
  if (lane == 0) mask[wave] = word;
}

/* ---- x-pass: one voxel with x in the box per lane, every row of the extended box ------------------------------------------- */
__global__ __launch_bounds__(kDistThreads) void distance_x_kernel(DistGeom g, unsigned long long n, const unsigned long long* __restrict__ mask,
                                                                  int16_t* __restrict__ dx_out) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kDistThreads + threadIdx.x;
  if (i >= n) return;
  const unsigned long long row = i / g.dims[0];
  const uint32_t x = (uint32_t)(i % g.dims[0]);
  dx_out[i] = (int16_t)dist_x_pass(mask + row * g.W, x + g.R, g.R);
}

/* ---- y-pass and z-pass ------------------------------------------------------------------------------------------------------
 * One voxel per lane, lanes along x. The input is `outer` slabs of rows_out + 2R rows of `inner` elements, the output `outer`
 * slabs of rows_out rows: the y-pass has inner = dims[0] and a slab per level of the extended box, the z-pass inner = dims[0] x
 * dims[1] and one slab. kZ: the input is the y-pass's dword, otherwise the x-pass's dx. kFinal: d2, offsets and metres are written
 * (each may be nullptr), otherwise the dword (dx, dy). */
struct CostDx {
  const int16_t* p;
  long long stride;
  __device__ __forceinline__ uint32_t operator()(int32_t k) const { return dist_cost_dx((int32_t)p[k * stride]); }
};
struct CostDxy {
  const uint32_t* p;
  long long stride;
  __device__ __forceinline__ uint32_t operator()(int32_t k) const { return dist_cost_dxy(p[k * stride]); }
};

template <bool kZ, bool kFinal>
__global__ __launch_bounds__(kDistThreads) void distance_column_kernel(unsigned long long n, uint32_t inner, uint32_t rows_out, uint32_t R, uint32_t early,
                                                                       double leaf, const void* __restrict__ in, uint32_t* __restrict__ dxy_out,
                                                                       uint16_t* __restrict__ d2_out, int16_t* __restrict__ offset_out,
                                                                       float* __restrict__ metres_out) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kDistThreads + threadIdx.x;
  if (i >= n) return;
  const unsigned long long line = i / inner;  // o * rows_out + r
  const uint32_t j = (uint32_t)(i % inner);
  const unsigned long long o = line / rows_out;
  const uint32_t r = (uint32_t)(line % rows_out);
  const unsigned long long at = ((o * (rows_out + 2ull * R) + r + R) * inner) + j;  // the voxel's own row of the input
  int32_t k = 0;
  uint32_t best, dxy = kDistNoDxy;
  if (kZ) {
    const uint32_t* p = static_cast<const uint32_t*>(in) + at;
    best = dist_column_pass(CostDxy{p, (long long)inner}, R, early != 0u, k);
    if (best != kDistNone) dxy = p[(long long)k * inner];
  } else {
    const int16_t* p = static_cast<const int16_t*>(in) + at;
    best = dist_column_pass(CostDx{p, (long long)inner}, R, early != 0u, k);
    if (best != kDistNone) dxy = dist_pack((int32_t)p[(long long)k * inner], k);
  }
  if (!kFinal) {
    dxy_out[i] = dxy;
    return;
  }
  const bool far = best == kDistNone;
  const uint32_t d2 = far ? kDistFar : best;
  if (d2_out) d2_out[i] = (uint16_t)d2;
  if (offset_out) {
    const bool zero = far || best == 0u;
    if (kZ) {
      offset_out[3 * i] = (int16_t)(zero ? 0 : dist_dx(dxy)), offset_out[3 * i + 1] = (int16_t)(zero ? 0 : dist_dy(dxy));
      offset_out[3 * i + 2] = (int16_t)(zero ? 0 : k);
    } else {
      offset_out[2 * i] = (int16_t)(zero ? 0 : dist_dx(dxy)), offset_out[2 * i + 1] = (int16_t)(zero ? 0 : k);
    }
  }
  if (metres_out) metres_out[i] = dist_metres(d2, leaf);
}

inline dim3 dist_blocks(unsigned long long n) { return dim3((uint32_t)((n + kDistThreads - 1) / kDistThreads)); }

}  // namespace

DistGeom make_dist_geom(const int32_t* vmin, const uint32_t* dims, uint32_t R, bool unknown_is_obstacle, bool slice) {
  DistGeom g;
  for (int a = 0; a < 3; a++) g.vmin[a] = vmin[a], g.dims[a] = dims[a];
  g.R = R, g.unknown_is_obstacle = unknown_is_obstacle ? 1u : 0u, g.slice = slice ? 1u : 0u;
  g.levels = dims[2];
  g.e[0] = dims[0] + 2u * R, g.e[1] = dims[1] + 2u * R, g.e[2] = slice ? 1u : dims[2] + 2u * R;
  g.W = (g.e[0] + 63u) / 64u;
  return g;
}

DistStaging dist_staging_carve(void* block, const DistGeom& g, size_t* bytes) {
  const unsigned long long rows = (unsigned long long)g.e[1] * g.e[2];
  const size_t b_mask = align256((size_t)(rows * g.W) * sizeof(unsigned long long));
  const size_t b_dx = align256((size_t)(rows * g.dims[0]) * sizeof(int16_t));
  const size_t b_dxy = g.slice ? 0 : align256((size_t)g.e[2] * g.dims[1] * g.dims[0] * sizeof(uint32_t));
  char* b = static_cast<char*>(block);
  DistStaging s;
  s.mask = reinterpret_cast<unsigned long long*>(b), s.dx = reinterpret_cast<int16_t*>(b + b_mask);
  s.dxy = reinterpret_cast<uint32_t*>(b + b_mask + b_dx);
  if (bytes) *bytes = b_mask + b_dx + b_dxy;
  return s;
}

void launch_distance(const OccTable& t, const OccStateRule& sr, double leaf, const DistGeom& g, const DistStaging& w, bool early, uint16_t* d_d2_out,
                     int16_t* d_offset_out, float* d_metres_out, hipStream_t s) {
  const unsigned long long rows = (unsigned long long)g.e[1] * g.e[2], n_waves = rows * g.W;
  for (unsigned long long w0 = 0; w0 < n_waves; w0 += kDistMaskWavesPerLaunch) {
    const unsigned long long nw = n_waves - w0 < kDistMaskWavesPerLaunch ? n_waves - w0 : kDistMaskWavesPerLaunch;
    const dim3 grid((uint32_t)((nw + kDistThreads / 64 - 1) / (kDistThreads / 64)));
    if (g.slice) launch_kernel(distance_mask_kernel<true>, grid, dim3(kDistThreads), 0, s, t, sr, g, w0, n_waves, w.mask);
    else launch_kernel(distance_mask_kernel<false>, grid, dim3(kDistThreads), 0, s, t, sr, g, w0, n_waves, w.mask);
  }
  const unsigned long long n_x = rows * g.dims[0];
  launch_kernel(distance_x_kernel, dist_blocks(n_x), dim3(kDistThreads), 0, s, g, n_x, w.mask, w.dx);
  const uint32_t e = early ? 1u : 0u;
  if (g.slice) {
    const unsigned long long n = (unsigned long long)g.dims[0] * g.dims[1];
    launch_kernel((distance_column_kernel<false, true>), dist_blocks(n), dim3(kDistThreads), 0, s, n, g.dims[0], g.dims[1], g.R, e, leaf,
                  static_cast<const void*>(w.dx), static_cast<uint32_t*>(nullptr), d_d2_out, d_offset_out, d_metres_out);
    return;
  }
  const unsigned long long plane = (unsigned long long)g.dims[0] * g.dims[1], n_y = plane * g.e[2], n = plane * g.dims[2];
  launch_kernel((distance_column_kernel<false, false>), dist_blocks(n_y), dim3(kDistThreads), 0, s, n_y, g.dims[0], g.dims[1], g.R, e, leaf,
                static_cast<const void*>(w.dx), w.dxy, static_cast<uint16_t*>(nullptr), static_cast<int16_t*>(nullptr), static_cast<float*>(nullptr));
  launch_kernel((distance_column_kernel<true, true>), dist_blocks(n), dim3(kDistThreads), 0, s, n, (uint32_t)plane, g.dims[2], g.R, e, leaf,
                static_cast<const void*>(w.dxy), static_cast<uint32_t*>(nullptr), d_d2_out, d_offset_out, d_metres_out);
}

}  // namespace loamx
