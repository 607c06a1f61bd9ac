// cloudmap_kernels.hip — the cloud map (loamx.h, "cloud map"): posed clouds accumulated on a voxel grid as integer sums, the
// voxel list in order of first appearance, and the centroids read out in that order. Per-point arithmetic: cloudmap_math.h.
// What this unit adds to the listed voxel table it shares with the surfel map: its payload for the accumulate kernel
// (listed_accumulate.h) and the scatter of its emit (behind the flags of listed_kernels.hip, where the launches of an add and of an
// emit are counted out).
#include "listed_accumulate.h"
#include "map_compact.h"

namespace loamx {
namespace {

// a slot holds the three sums of the points' offsets inside the voxel (the pose's origin is not used)
struct CloudPayload {
  static constexpr int kWords = (int)kCloudSlotWords;
  static __device__ __forceinline__ void point(const uint32_t u[3], Vec3, Vec3, double, unsigned long long m[kWords]) {
    for (int a = 0; a < 3; a++) m[a] = u[a];
  }
};

// one flagged list entry per thread: its centroid, count and first point to the entry's place in the output
__global__ __launch_bounds__(kListedThreads) void cloud_emit_scatter_kernel(const uint8_t* __restrict__ keep, const uint32_t* __restrict__ tiles, ListedTable t,
                                                                           double leaf, unsigned long long capacity, double* __restrict__ xyz_out,
                                                                           uint32_t* __restrict__ count_out, uint32_t* __restrict__ first_out) {
  __shared__ uint32_t s_wave[4];
  const uint32_t j = blockIdx.x * kListedThreads + threadIdx.x;
  const bool flag = j < t.max_voxels && keep[j] != 0;
  uint32_t total;
  const uint32_t rank = block_rank(flag, s_wave, total);
  if (!flag) return;
  const uint32_t dst = tiles[blockIdx.x] + rank;
  if (dst >= capacity) return;
  const uint32_t s = t.list[j], cnt = t.count[s];
  const uint64_t key = t.keys[s];
  for (int a = 0; a < 3; a++) xyz_out[(size_t)dst * 3 + a] = cloud_centroid(cloud_key_coord(key, a), t.payload[(size_t)s * kCloudSlotWords + a], cnt, leaf);
  if (count_out) count_out[dst] = cnt;
  if (first_out) first_out[dst] = t.first[s];
}

}  // namespace

void launch_cloud_accumulate(const void* d_points, bool f32, uint32_t stride, const OrgOffsets& offs, uint32_t n_clouds, unsigned long long p0,
                             uint32_t n, uint32_t g0, const double* d_poses, const CloudRule& rule, const ListedTable& t, bool combine, uint32_t* d_slot,
                             hipStream_t s) {
  launch_listed_accumulate<CloudPayload>(d_points, f32, stride, offs, n_clouds, p0, n, g0, d_poses, rule, t, combine, d_slot, s);
}

void launch_cloud_emit(const ListedTable& t, double leaf, uint32_t min_points, uint8_t* d_keep, uint32_t* d_tiles, double* d_xyz_out,
                       uint32_t* d_count_out, uint32_t* d_first_out, size_t capacity, uint32_t* d_n_out, hipStream_t s) {
  launch_listed_emit_flags(t, min_points, d_keep, d_tiles, d_n_out, s);
  launch_kernel(cloud_emit_scatter_kernel, listed_tiles(t.max_voxels), dim3(kListedThreads), 0, s, (const uint8_t*)d_keep, (const uint32_t*)d_tiles, t, leaf,
                (unsigned long long)capacity, d_xyz_out, d_count_out, d_first_out);
}

}  // namespace loamx
