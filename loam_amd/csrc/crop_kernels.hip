// crop_kernels.hip — the map window (loamx.h, "map window"): the voxels of a cloud map, a surfel map or an occupancy map outside a
// box around a device pose leave the map. The rule: crop_math.h; the stable compaction is the one of map_kernels.hip
// (map_compact.h); the claim is the table's own (voxel_table.h).
//
// The rule of the table forbids taking a key out of its slot, and an emptied slot in the middle of a probe chain would make
// voxel_find stop early for every key behind it. So a crop REBUILDS the table, in six launches: flags over the entries (the list
// of a listed map, the slots of the occupancy map), the two launches of the compaction's tile offsets, a gather of the kept voxels
// into a dense staging array in entry order, a reset of the table arrays to their empty state, and a scatter that claims a slot
// for every staged key, writes its payload and its list entry, and commits the new length. No launch waits for another workgroup,
// there is no floating-point atomic, and every loop has a bound that does not depend on the data.
//
// A skipped crop (a centre that is not finite) raises one control word in the flags launch; gather, reset and scatter return on
// that word before they touch anything, so the map keeps every byte.
#include "crop_math.h"
#include "loamx_internal.h"
#include "map_compact.h"
#include "voxel_table.h"

namespace loamx {
namespace {

constexpr int kCropThreads = (int)kMapTile;  // one entry per thread; the tiles of the compaction are the workgroups

struct CropBox {
  double lo[3], hi[3];
};

// Entry j is kept iff it holds a voxel and the rule keeps its key. The centre comes from the device pose by loads whose address is
// the same in every lane (the compiler makes them scalar loads: the centre, the box and the leaf sit in scalar registers), so the
// bounds and the skip decision are the same in every thread of the launch (FP64 has no scalar ALU here: the six quotients are
// formed per lane, from uniform operands); thread 0 leaves the decision in ctl for the launches behind. A skipped crop flags every voxel, so that the compaction's total is the
// map's voxel count. Plain loads of the keys: this launch claims nothing.
__global__ __launch_bounds__(kCropThreads) void crop_flags_kernel(CropTable t, double leaf, const double* __restrict__ pose, CropBox box,
                                                                  uint8_t* __restrict__ keep, uint32_t* __restrict__ ctl) {
  const uint32_t j = blockIdx.x * kCropThreads + threadIdx.x;
  if (j >= t.entries) return;
  double c[3] = {0.0, 0.0, 0.0};
  if (pose)
    for (int a = 0; a < 3; a++) c[a] = pose[4 + a];
  const bool skip = crop_skips(c);
  const CropBounds b = crop_bounds(c, box.lo, box.hi, leaf);
  if (j == 0) ctl[kCropCtlSkip] = skip ? 1u : 0u;
  bool on;
  unsigned long long key = 0;
  if (t.list) {
    on = j < *t.listed;
    if (on) key = t.keys[t.list[j]];
  } else {
    key = t.keys[j];
    on = key != kVoxelEmpty;
  }
  keep[j] = on && (skip || crop_keeps(key, b));
}

// the kept entries' key, payload, first and count to their position in entry order; thread 0 writes the counts word
// {kept, removed, skipped, 0}. The staged payload is laid out [word][entry]: the stores here and the loads of the scatter are
// contiguous over the lanes, the table's side is an indexed access in both.
__global__ __launch_bounds__(kCropThreads) void crop_gather_kernel(CropTable t, CropScratch w, uint32_t* __restrict__ counts_out) {
  __shared__ uint32_t s_wave[4];
  const uint32_t j = blockIdx.x * kCropThreads + threadIdx.x;
  const uint32_t skip = w.ctl[kCropCtlSkip], kept = w.ctl[kCropCtlKept];
  if (j == 0 && counts_out) {
    const uint32_t before = t.list ? *t.listed : (uint32_t)*t.voxels;
    counts_out[0] = skip ? before : kept, counts_out[1] = skip ? 0u : before - kept, counts_out[2] = skip, counts_out[3] = 0u;
  }
  if (skip) return;  // (uniform over the launch)
  const bool flag = j < t.entries && w.keep[j] != 0;
  uint32_t total;
  const uint32_t rank = block_rank(flag, s_wave, total);
  if (!flag) return;
  const uint32_t dst = w.tiles[blockIdx.x] + rank, s = t.list ? t.list[j] : j;
  w.keys[dst] = t.keys[s];
  for (uint32_t k = 0; k < t.payload_words; k++) w.payload[(size_t)k * t.entries + dst] = t.payload[(size_t)s * t.payload_words + k];
  if (t.first) w.first[dst] = t.first[s];
  if (t.count) w.count[dst] = t.count[s];
}

// The table arrays alone back to their empty state (keys and first all ones, payload and counts zero: atomicMin on first and the
// adds on the sums rely on it), never the counter words or the lengths. One thread per slot; the payload is cleared as one flat
// array, word k * cap + slot, so that the lanes' stores are contiguous.
__global__ __launch_bounds__(kCropThreads) void crop_reset_kernel(CropTable t, const uint32_t* __restrict__ ctl) {
  if (ctl[kCropCtlSkip]) return;  // (uniform over the launch)
  const size_t cap = (size_t)1 << t.log2_cap, s = (size_t)blockIdx.x * kCropThreads + threadIdx.x;
  if (s >= cap) return;
  t.keys[s] = kVoxelEmpty;
  for (uint32_t k = 0; k < t.payload_words; k++) t.payload[(size_t)k * cap + s] = 0ull;
  if (t.first) t.first[s] = 0xFFFFFFFFu;
  if (t.count) t.count[s] = 0u;
}

// Staged entry i claims its slot by the rule of the table (every probe a 64-bit CAS, no plain load of a key slot in this launch),
// writes its payload with plain stores (keys are distinct, so it is the only writer of that slot) and sets list[i]. The claim can
// never give up: at most as many keys as the table held go into an empty table of the same size. Thread 0 commits the new length
// (no thread of this launch reads it).
__global__ __launch_bounds__(kCropThreads) void crop_scatter_kernel(CropTable t, CropScratch w) {
  if (w.ctl[kCropCtlSkip]) return;  // (uniform over the launch)
  const uint32_t i = blockIdx.x * kCropThreads + threadIdx.x, kept = w.ctl[kCropCtlKept];
  if (i == 0) {
    if (t.list) *t.listed = kept;
    else *t.voxels = kept;
  }
  if (i >= kept || i >= t.entries) return;
  bool opened;
  const uint32_t slot = voxel_claim(t.keys, t.log2_cap, w.keys[i], opened);
  if (slot == kMapNoSlot) return;
  for (uint32_t k = 0; k < t.payload_words; k++) t.payload[(size_t)slot * t.payload_words + k] = w.payload[(size_t)k * t.entries + i];
  if (t.first) t.first[slot] = w.first[i];
  if (t.count) t.count[slot] = w.count[i];
  if (t.list) t.list[i] = slot;
}

inline dim3 crop_tiles(size_t n) { return dim3((unsigned)((n + kMapTile - 1) / kMapTile)); }

struct CropLayout {
  size_t o_tiles, o_ctl, o_keys, o_payload, o_first, o_count, bytes;
};
inline CropLayout crop_layout(const CropTable& t) {
  CropLayout l;
  const size_t n = t.entries;
  l.o_tiles = align256(n);
  l.o_ctl = l.o_tiles + align256(map_compact_ws_bytes(n));
  l.o_keys = l.o_ctl + align256(kCropCtlWords * sizeof(uint32_t));
  l.o_payload = l.o_keys + align256(n * sizeof(unsigned long long));
  l.o_first = l.o_payload + align256(n * t.payload_words * sizeof(unsigned long long));
  l.o_count = l.o_first + (t.first ? align256(n * sizeof(uint32_t)) : 0);  // (a table without first and count stages none)
  l.bytes = l.o_count + (t.count ? align256(n * sizeof(uint32_t)) : 0);
  return l;
}

}  // namespace

size_t crop_scratch_bytes(const CropTable& t) { return crop_layout(t).bytes; }

CropScratch crop_scratch_carve(void* block, const CropTable& t) {
  const CropLayout l = crop_layout(t);
  char* b = static_cast<char*>(block);
  CropScratch w;
  w.keep = reinterpret_cast<uint8_t*>(b), w.tiles = reinterpret_cast<uint32_t*>(b + l.o_tiles), w.ctl = reinterpret_cast<uint32_t*>(b + l.o_ctl);
  w.keys = reinterpret_cast<unsigned long long*>(b + l.o_keys), w.payload = reinterpret_cast<unsigned long long*>(b + l.o_payload);
  w.first = reinterpret_cast<uint32_t*>(b + l.o_first), w.count = reinterpret_cast<uint32_t*>(b + l.o_count);
  return w;
}

void launch_voxel_crop(const CropTable& t, const CropScratch& w, double leaf, const double* d_pose, const double lo[3], const double hi[3],
                       uint32_t* d_counts_out, hipStream_t s) {
  CropBox box;
  for (int a = 0; a < 3; a++) box.lo[a] = lo[a], box.hi[a] = hi[a];
  launch_kernel(crop_flags_kernel, crop_tiles(t.entries), dim3(kCropThreads), 0, s, t, leaf, d_pose, box, w.keep, w.ctl);
  launch_tile_offsets(w.keep, t.entries, w.tiles, w.ctl + kCropCtlKept, s);
  launch_kernel(crop_gather_kernel, crop_tiles(t.entries), dim3(kCropThreads), 0, s, t, w, d_counts_out);
  launch_kernel(crop_reset_kernel, crop_tiles((size_t)1 << t.log2_cap), dim3(kCropThreads), 0, s, t, (const uint32_t*)w.ctl);
  launch_kernel(crop_scatter_kernel, crop_tiles(t.entries), dim3(kCropThreads), 0, s, t, w);
}

}  // namespace loamx
