// map_kernels.hip — upkeep of a local map held in a persistent target index (loamx.h, "map upkeep"): the voxel filter of
// new points against an occupancy table (loamx_voxel_filter_dev, loamx_target_index_insert_filtered), the box test of the
// crop (loamx_target_index_crop) and the stable compaction all three share. Per-point arithmetic: map_math.h.
#include "loamx_internal.h"
#include "map_compact.h"
#include "map_math.h"
#include "voxel_table.h"

namespace loamx {
namespace {

constexpr int kMapThreads = (int)kMapTile;  // one point per thread, one tile per workgroup

struct Pose7 {
  double v[7];
};
struct Box3 {
  double lo[3], hi[3];
};

__device__ __forceinline__ Vec3 load_point(const double* __restrict__ pts, uint32_t i) {
  const double* p = pts + (size_t)i * 3;
  return v3(p[0], p[1], p[2]);
}
__device__ __forceinline__ void store_point(double* __restrict__ pts, uint32_t i, Vec3 p) {
  double* o = pts + (size_t)i * 3;
  o[0] = p.x, o[1] = p.y, o[2] = p.z;
}

/* ---- claim ---------------------------------------------------------------------------------------------------------
 * One thread per point: p' = pose.act(p) (skipped for the identity), key of its voxel, then the claim of its slot under the
 * rule of voxel_table.h (voxel_claim). The winner of a voxel is the LOWEST point index (atomicMin on the slot's owner word), so
 * the outcome does not depend on which thread came first. A probe that gave up raises flags[kMapFlagGaveUp]; a point without a
 * voxel (non-finite, or out of range) raises flags[bad_word].
 * moved / slot_out may be null (the points of the map itself, when a table is built or caught up). */
__global__ __launch_bounds__(kMapThreads) void voxel_claim_kernel(const double* __restrict__ pts, uint32_t n, Pose7 pose, uint32_t identity, double leaf,
                                                                   unsigned long long* keys, uint32_t* owner, uint32_t log2_cap, uint32_t base,
                                                                   double* __restrict__ moved, uint32_t* __restrict__ slot_out, uint32_t* flags,
                                                                   uint32_t bad_word) {
  const uint32_t i = blockIdx.x * kMapThreads + threadIdx.x;
  if (i >= n) return;
  Vec3 p = load_point(pts, i);
  if (!identity) p = pose_act(pose.v, p);
  if (moved) store_point(moved, i, p);
  uint32_t slot = kMapNoSlot;
  uint64_t key;
  if (voxel_key(p, leaf, key)) {
    bool opened;
    slot = voxel_claim(keys, log2_cap, key, opened);
    if (slot != kMapNoSlot) atomicMin(owner + slot, base + i);
    else atomicOr(flags + kMapFlagGaveUp, 1u);
  } else {
    atomicOr(flags + bad_word, 1u);
  }
  if (slot_out) slot_out[i] = slot;
}

// second launch (plain loads are fine across the kernel boundary): a point is kept iff it owns its voxel
__global__ __launch_bounds__(kMapThreads) void voxel_keep_kernel(const uint32_t* __restrict__ owner, const uint32_t* __restrict__ slot, uint32_t n,
                                                                  uint32_t base, uint8_t* __restrict__ keep) {
  const uint32_t i = blockIdx.x * kMapThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = slot[i];
  keep[i] = s != kMapNoSlot && owner[s] == base + i;
}

__global__ __launch_bounds__(kMapThreads) void crop_keep_kernel(const double* __restrict__ pts, uint32_t n, Box3 box, uint8_t* __restrict__ keep) {
  const uint32_t i = blockIdx.x * kMapThreads + threadIdx.x;
  if (i >= n) return;
  keep[i] = box_holds(load_point(pts, i), box.lo, box.hi);
}

// leaf <= 0: the transform alone. Every point is kept, so out[i] belongs to point i and the count is n.
__global__ __launch_bounds__(kMapThreads) void map_transform_kernel(const double* __restrict__ pts, uint32_t n, Pose7 pose, uint32_t identity,
                                                                     double* __restrict__ out, uint32_t* __restrict__ src_idx, uint32_t* __restrict__ n_out,
                                                                     uint32_t* flags) {
  const uint32_t i = blockIdx.x * kMapThreads + threadIdx.x;
  if (i == 0) *n_out = n;
  if (i >= n) return;
  Vec3 p = load_point(pts, i);
  if (!identity) p = pose_act(pose.v, p);
  store_point(out, i, p);
  if (src_idx) src_idx[i] = i;
  if (flags && !((p.x + p.y + p.z) * 0.0 == 0.0)) atomicOr(flags + kMapFlagBadPoint, 1u);
}

/* ---- stable compaction -----------------------------------------------------------------------------------------------
 * Three launches over tiles of kMapTile points, none of which waits for another workgroup: counts of the kept points per
 * tile; ONE workgroup turns the counts into the tiles' first output positions (it walks the tiles 256 at a time with a
 * running total, so any number of tiles takes the same code) and writes the total; every tile then ranks its kept points
 * again and moves them to base[tile] + rank. Kept points therefore leave in input order. block_rank and the launcher of the
 * first two launches stand in map_compact.h: the cloud map (cloudmap_kernels.hip) compacts with them too. */
__global__ __launch_bounds__(kMapThreads) void tile_count_kernel(const uint8_t* __restrict__ keep, uint32_t n, uint32_t* __restrict__ tiles) {
  __shared__ uint32_t s_wave[4];
  const uint32_t i = blockIdx.x * kMapThreads + threadIdx.x;
  uint32_t total;
  (void)block_rank(i < n && keep[i] != 0, s_wave, total);
  if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

// tiles[t]: count -> first output position of tile t (in place: a thread reads its entry before it writes it)
__global__ __launch_bounds__(kMapThreads) void tile_scan_kernel(uint32_t* __restrict__ tiles, uint32_t n_tiles, uint32_t* __restrict__ total_out) {
  __shared__ uint32_t s_wave[4];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  uint32_t carry = 0;
  for (uint32_t t0 = 0; t0 < n_tiles; t0 += kMapThreads) {
    const uint32_t t = t0 + threadIdx.x;
    const uint32_t c = t < n_tiles ? tiles[t] : 0u;
    uint32_t incl = c;  // inclusive scan inside the wavefront
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[w] = incl;
    __syncthreads();
    uint32_t before = 0, chunk = 0;
    for (uint32_t j = 0; j < 4; j++) {
      const uint32_t s = s_wave[j];
      before += j < w ? s : 0u;
      chunk += s;
    }
    if (t < n_tiles) tiles[t] = carry + before + incl - c;
    carry += chunk;
    __syncthreads();  // (s_wave is written again by the next round)
  }
  if (threadIdx.x == 0) *total_out = carry;
}

// owner != null (the filtered insert): a kept point will sit at index owner_base + position in the map, which is what the
// table's invariant says its voxel's owner word holds (it held owner_base + input index, never smaller)
__global__ __launch_bounds__(kMapThreads) void tile_scatter_kernel(const double* __restrict__ in, const uint8_t* __restrict__ keep, uint32_t n,
                                                                    const uint32_t* __restrict__ tiles, double* __restrict__ out,
                                                                    uint32_t* __restrict__ src_idx, uint32_t* owner, const uint32_t* __restrict__ slot,
                                                                    uint32_t owner_base) {
  __shared__ uint32_t s_wave[4];
  const uint32_t i = blockIdx.x * kMapThreads + threadIdx.x;
  const bool flag = i < n && keep[i] != 0;
  uint32_t total;
  const uint32_t rank = block_rank(flag, s_wave, total);
  if (!flag) return;
  const uint32_t dst = tiles[blockIdx.x] + rank;
  store_point(out, dst, load_point(in, i));
  if (src_idx) src_idx[dst] = i;
  if (owner) owner[slot[i]] = owner_base + dst;
}

inline Pose7 pose7(const double* pose) {
  Pose7 P{{0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0}};
  if (pose)
    for (int k = 0; k < 7; k++) P.v[k] = pose[k];
  return P;
}
inline dim3 tiles_of(uint32_t n) { return dim3((n + kMapTile - 1) / kMapTile); }

}  // namespace

// pose == nullptr: identity (no arithmetic at all). Every launcher below is a no-op for n == 0 unless it says otherwise.
void launch_voxel_claim(const double* d_pts, uint32_t n, const double* pose, double leaf, const VoxelTable& t, uint32_t base, double* d_moved,
                        uint32_t* d_slot, uint32_t* d_flags, uint32_t bad_word, hipStream_t s) {
  if (n == 0) return;
  launch_kernel(voxel_claim_kernel, tiles_of(n), dim3(kMapThreads), 0, s, d_pts, n, pose7(pose), pose ? 0u : 1u, leaf, t.keys, t.owner, t.log2_cap, base,
                d_moved, d_slot, d_flags, bad_word);
}

void launch_voxel_keep(const VoxelTable& t, const uint32_t* d_slot, uint32_t n, uint32_t base, uint8_t* d_keep, hipStream_t s) {
  if (n == 0) return;
  launch_kernel(voxel_keep_kernel, tiles_of(n), dim3(kMapThreads), 0, s, (const uint32_t*)t.owner, d_slot, n, base, d_keep);
}

void launch_crop_keep(const double* d_pts, uint32_t n, const double lo[3], const double hi[3], uint8_t* d_keep, hipStream_t s) {
  if (n == 0) return;
  Box3 b;
  for (int c = 0; c < 3; c++) b.lo[c] = lo[c], b.hi[c] = hi[c];
  launch_kernel(crop_keep_kernel, tiles_of(n), dim3(kMapThreads), 0, s, d_pts, n, b, d_keep);
}

// writes *d_n_out = n also for n == 0; d_flags may be null (a non-finite result is then not reported)
void launch_map_transform(const double* d_pts, uint32_t n, const double* pose, double* d_out, uint32_t* d_src_idx, uint32_t* d_n_out,
                          uint32_t* d_flags, hipStream_t s) {
  launch_kernel(map_transform_kernel, n ? tiles_of(n) : dim3(1), dim3(kMapThreads), 0, s, d_pts, n, pose7(pose), pose ? 0u : 1u, d_out, d_src_idx, d_n_out,
                d_flags);
}

void launch_tile_offsets(const uint8_t* d_keep, uint32_t n, uint32_t* d_tiles, uint32_t* d_total, hipStream_t s) {
  const uint32_t n_tiles = (n + kMapTile - 1) / kMapTile;
  if (n) launch_kernel(tile_count_kernel, dim3(n_tiles), dim3(kMapThreads), 0, s, d_keep, n, d_tiles);
  launch_kernel(tile_scan_kernel, dim3(1), dim3(kMapThreads), 0, s, d_tiles, n_tiles, d_total);
}

size_t map_compact_ws_bytes(size_t n) { return ((n + kMapTile - 1) / kMapTile + 1) * sizeof(uint32_t); }

// d_out: room for n points; d_tiles: map_compact_ws_bytes(n). Writes *d_total also for n == 0.
void launch_map_compact(const double* d_in, const uint8_t* d_keep, uint32_t n, uint32_t* d_tiles, double* d_out, uint32_t* d_src_idx,
                        uint32_t* d_total, const VoxelTable* fix, const uint32_t* d_slot, uint32_t owner_base, hipStream_t s) {
  launch_tile_offsets(d_keep, n, d_tiles, d_total, s);
  if (n)
    launch_kernel(tile_scatter_kernel, tiles_of(n), dim3(kMapThreads), 0, s, d_in, d_keep, n, (const uint32_t*)d_tiles, d_out, d_src_idx,
                  fix ? fix->owner : (uint32_t*)nullptr, d_slot, owner_base);
}

}  // namespace loamx
