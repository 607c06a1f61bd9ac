// segment_kernels.hip — scan segmentation (loamx.h: loamx_segment_scans_dev; the rule per cell and per pair: segment_math.h).
// Connected components of a cylindrical H x W image per scan, blockIdx.y = scan. Seven launches, separated by kernel boundaries
// only: no flag, no spin-wait, nothing one workgroup waits on another for.
//   classify   one thread per cell: validity of the cell and of its line neighbours, the (at most two) ground pairs. Writes the
//              cell's first class (invalid / ground / node) and resets the words the later stages accumulate at a root.
//   edges      one workgroup per tile of kSegTileLines x kSegTileCols cells, a thread per column walking the lines: the edge
//              predicate once per node and direction (points are only loaded where both ends are nodes). Tile form: labels of the
//              tile in LDS (16 KB); a cell starts at the first cell of its run of connected cells inside the wavefront's 64
//              columns (one ballot), the remaining edges inside the tile go through a union-find in LDS (atomicMin on the larger
//              root: only the minimum wins), then every cell is flattened to its tile root and ONE global parent is written. The
//              connected edges that leave the tile (and the seam edge, whatever the tile) are left as two bits per cell.
//              Global-only form (context option NO_SEGMENT_TILES): parent = the cell itself, every connected edge is left as a bit.
//   merge      one thread per cell: the edges left as bits go through a union on the global parents. atomicMin on the larger
//              root with a retry on the old value; parents are read with relaxed agent-scope atomic loads (other workgroups are
//              changing them; a plain load may be served from this CU's L1).
//   flatten    one thread per cell: walks to its root (parents no longer change: plain loads behind the kernel boundary), writes
//              it, and adds the cell to the root's size and line maximum — once per run of lanes with the same root, not per lane
//              (cells of a line are neighbours in a wavefront). The line minimum needs no word: the root is the smallest index.
//   decide     one thread per cell: accept rule from the root's words, classes, labels, sizes, the filtered copy; the stats and
//              the accepted roots per block of 256 cells by ballot, one LDS word each, then one global atomic per block and word.
//   finish     one workgroup per scan: exclusive prefix sum of the accepted roots per block, the stats record.
//   clusters   one thread per cell: accepted roots to their position = the block's prefix + the rank inside the block
//              (map_compact.h): ascending root order, from an ordered compaction.
// Every loop is bounded: a parent is smaller than its cell (LDS: local index; global: linear index), so a walk from x takes at most
// x steps, and a union retries only after some parent has decreased.
// Algorithmic bytes per cell (f64; f32: 12 B per point): classify 24 B read (+ the line neighbours from cache) + 10 B written;
// edges 2 B read, 1 B + 4 B per node written, 24 B per node with a node neighbour read again; merge 1 B; flatten 5 B read, 4 B
// written; decide 9 B + 24 B read, 1 + 4 + 4 + 24 B written.
#include "loamx_internal.h"
#include "map_compact.h"

namespace loamx {
namespace {

constexpr uint32_t TL = kSegTileLines, TC = kSegTileCols;
static_assert(TL <= 32, "one bit per line of the tile in a 32-bit mask");
static_assert(TC == 256 && kSegBlock == 256, "four wavefronts per workgroup");

template <typename T>
__device__ __forceinline__ void seg_load(const T* scan, size_t cell, double& x, double& y, double& z) {
  const T* p = scan + cell * 3;
  x = (double)p[0], y = (double)p[1], z = (double)p[2];
}

template <typename T>
__global__ __launch_bounds__(kSegBlock) void segment_classify_kernel(const T* __restrict__ scans, SegParams P, SegScratch ws) {
  const uint32_t HW = P.H * P.W;
  const uint32_t i = blockIdx.x * kSegBlock + threadIdx.x;
  if (i >= HW) return;
  const size_t base = (size_t)blockIdx.y * HW;
  const T* scan = scans + base * 3;
  double x, y, z;
  seg_load(scan, i, x, y, z);
  uint8_t c = kSegInvalid;
  if (seg_valid(x, y, z, P.min_range, P.max_range)) {
    const uint32_t l = i / P.W;
    bool ground = false;
    if (l + 1 < P.G) {  // the pair (l, l + 1)
      double ux, uy, uz;
      seg_load(scan, (size_t)i + P.W, ux, uy, uz);
      ground = seg_valid(ux, uy, uz, P.min_range, P.max_range) && seg_ground_pair(x, y, z, ux, uy, uz, P.tg2);
    }
    if (!ground && l >= 1 && l < P.G) {  // the pair (l - 1, l)
      double dx, dy, dz;
      seg_load(scan, (size_t)i - P.W, dx, dy, dz);
      ground = seg_valid(dx, dy, dz, P.min_range, P.max_range) && seg_ground_pair(dx, dy, dz, x, y, z, P.tg2);
    }
    c = ground ? kSegGround : kSegNode;
  }
  ws.cls[base + i] = c;
  ws.size[base + i] = 0u;
  ws.line_max[base + i] = 0u;
}

/* ---- union-find in LDS (labels are local indices ll TC + column; only nodes are ever looked up) ---------------------------- */
__device__ __forceinline__ uint32_t lds_find(uint32_t* L, uint32_t x) {
  for (;;) {
    const uint32_t p = __hip_atomic_load(L + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == x) return x;
    x = p;  // p < x
  }
}
__device__ __forceinline__ void lds_union(uint32_t* L, uint32_t a, uint32_t b) {
  for (;;) {
    a = lds_find(L, a), b = lds_find(L, b);
    if (a == b) return;
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const uint32_t old = atomicMin(L + hi, lo);
    if (old == hi) return;
    a = old, b = lo;  // hi had found another parent meanwhile (old < hi): join that one with lo
  }
}

/* ---- union-find on the global parents of one scan ---------------------------------------------------------------------------- */
__device__ __forceinline__ uint32_t seg_parent(const uint32_t* parent, uint32_t x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t global_find(uint32_t* parent, uint32_t x) {
  const uint32_t x0 = x;
  uint32_t hops = 0;
  for (;;) {
    const uint32_t p = seg_parent(parent, x);
    if (p == x) break;
    x = p, hops++;  // p < x
  }
  if (hops > 1) atomicMin(parent + x0, x);  // shorten the next walk from x0: x is an ancestor of x0 and below its parent
  return x;
}
__device__ __forceinline__ void global_union(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = global_find(parent, a), b = global_find(parent, b);
    if (a == b) return;
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const uint32_t old = atomicMin(parent + hi, lo);
    if (old == hi) return;
    a = old, b = lo;
  }
}

// blockIdx.x = tile of the scan (tile_cols tiles per row of tiles), thread = column of the tile
template <typename T, bool kTiles>
__global__ __launch_bounds__(TC) void segment_edges_kernel(const T* __restrict__ scans, SegParams P, SegScratch ws, uint32_t tile_cols) {
  __shared__ uint32_t s_lab[kTiles ? TL * TC : 1];
  __shared__ uint32_t s_handed;
  const uint32_t t = threadIdx.x, lane = t & 63u;
  const uint32_t l0 = (blockIdx.x / tile_cols) * TL, c0 = (blockIdx.x % tile_cols) * TC, c = c0 + t;
  const uint32_t HW = P.H * P.W;
  const size_t base = (size_t)blockIdx.y * HW;
  const T* scan = scans + base * 3;
  const uint8_t* cls = ws.cls + base;
  const bool col_in = c < P.W;
  const uint32_t cr = c + 1 == P.W ? 0u : c + 1;  // the right neighbour's column: the scan is a cylinder
  if (t == 0) s_handed = 0u;
  uint32_t rin_mask = 0, uin_mask = 0, node_mask = 0, handed = 0;
#pragma unroll
  for (uint32_t ll = 0; ll < TL; ll++) {
    const uint32_t l = l0 + ll;
    const bool in = col_in && l < P.H;
    const uint32_t i = l * P.W + c;
    const bool node = in && cls[i] == kSegNode;
    bool conn_r = false, conn_u = false;
    if (node) {
      const bool rn = P.W > 1 && cls[l * P.W + cr] == kSegNode;
      const bool un = l + 1 < P.H && cls[i + P.W] == kSegNode;
      if (rn || un) {
        double x, y, z, bx, by, bz;
        seg_load(scan, i, x, y, z);
        if (rn) {
          seg_load(scan, (size_t)l * P.W + cr, bx, by, bz);
          conn_r = seg_connected(x, y, z, bx, by, bz, P.c2);
        }
        if (un) {
          seg_load(scan, (size_t)i + P.W, bx, by, bz);
          conn_u = seg_connected(x, y, z, bx, by, bz, P.c2);
        }
      }
    }
    // inside the tile: the neighbour is a cell of this tile and the edge is not the seam's
    const bool rin = kTiles && conn_r && t + 1 < TC && c + 1 < P.W;
    const bool uin = kTiles && conn_u && ll + 1 < TL;
    const uint32_t eb = (conn_r && !rin ? 1u : 0u) | (conn_u && !uin ? 2u : 0u);
    if (in) ws.ebits[base + i] = (uint8_t)eb;
    handed += (eb & 1u) + (eb >> 1);
    if (kTiles) {
      rin_mask |= (rin ? 1u : 0u) << ll, uin_mask |= (uin ? 1u : 0u) << ll, node_mask |= (node ? 1u : 0u) << ll;
      // first lane of this lane's run of right-connected cells within the wavefront: the highest lane <= this one without a link
      // to its left neighbour (lane 0 never has one here: the link from the previous wavefront goes through the union below)
      const unsigned long long no_link = ~(__ballot(rin) << 1) & ((2ull << lane) - 1ull);
      const uint32_t start = 63u - (uint32_t)__clzll((long long)no_link);
      s_lab[ll * TC + t] = node ? ll * TC + (t - lane) + start : kSegNoLabel;
    } else if (node) {
      ws.parent[base + i] = i;
    }
  }
  __syncthreads();
  if (kTiles) {
#pragma unroll
    for (uint32_t ll = 0; ll < TL; ll++) {
      const bool rin = (rin_mask >> ll) & 1u, uin = (uin_mask >> ll) & 1u;
      const unsigned long long rb = __ballot(rin), ub = __ballot(uin), rb_up = __ballot((rin_mask >> (ll + 1)) & 1u);
      const uint32_t idx = ll * TC + t;
      if (rin && lane == 63u) lds_union(s_lab, idx, idx + 1);
      // an up edge whose left neighbour has one too, with both lines linked between the two columns, joins what that one joins
      const unsigned long long left = lane ? 1ull << (lane - 1) : 0ull;
      if (uin && !(ub & rb & rb_up & left)) lds_union(s_lab, idx, idx + TC);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t ll = 0; ll < TL; ll++) {
      if ((node_mask >> ll) & 1u) {
        const uint32_t r = lds_find(s_lab, ll * TC + t);
        ws.parent[base + (l0 + ll) * P.W + c] = (l0 + r / TC) * P.W + c0 + r % TC;
      }
    }
  }
  if (handed) atomicAdd(&s_handed, handed);
  __syncthreads();
  if (t == 0 && s_handed) atomicAdd(ws.edges + blockIdx.y, s_handed);
}

__global__ __launch_bounds__(kSegBlock) void segment_merge_kernel(SegParams P, SegScratch ws) {
  const uint32_t HW = P.H * P.W;
  const uint32_t i = blockIdx.x * kSegBlock + threadIdx.x;
  if (i >= HW) return;
  const size_t base = (size_t)blockIdx.y * HW;
  const uint32_t b = ws.ebits[base + i];
  if (!b) return;
  uint32_t* parent = ws.parent + base;
  if (b & 1u) global_union(parent, i, i % P.W + 1 == P.W ? i + 1 - P.W : i + 1);
  if (b & 2u) global_union(parent, i, i + P.W);
}

__global__ __launch_bounds__(kSegBlock) void segment_flatten_kernel(SegParams P, SegScratch ws) {
  const uint32_t HW = P.H * P.W;
  const uint32_t i = blockIdx.x * kSegBlock + threadIdx.x, lane = threadIdx.x & 63u;
  const size_t base = (size_t)blockIdx.y * HW;
  const bool in = i < HW;
  uint32_t r = kSegNoLabel;
  if (in && ws.cls[base + i] == kSegNode) {
    const uint32_t* parent = ws.parent + base;
    r = i;
    for (;;) {
      const uint32_t p = parent[r];
      if (p == r) break;
      r = p;  // p < r
    }
  }
  if (in) ws.root[base + i] = r;
  // one add per run of lanes with the same root
  const uint32_t prev = __shfl_up(r, 1);
  const bool head = lane == 0 || prev != r;
  const unsigned long long heads = __ballot(head);
  if (head && r != kSegNoLabel) {
    const unsigned long long after = (heads >> lane) >> 1;
    const uint32_t len = after ? (uint32_t)__ffsll((long long)after) : 64u - lane;
    atomicAdd(ws.size + base + r, len);
    atomicMax(ws.line_max + base + r, (i + len - 1) / P.W);  // the run's cells ascend: its last one lies on its highest line
  }
}

__device__ __forceinline__ void seg_count(uint32_t* word, bool flag) {
  const unsigned long long b = __ballot(flag);
  if ((threadIdx.x & 63u) == 0 && b) atomicAdd(word, (uint32_t)__popcll(b));
}

// (no __restrict__ on scans: out.filtered may be the input)
template <typename T>
__global__ __launch_bounds__(kSegBlock) void segment_decide_kernel(const T* scans, SegParams P, SegScratch ws, SegOutputs out, uint32_t nb) {
  __shared__ uint32_t s_c[kSegStatWords];
  if (threadIdx.x < kSegStatWords) s_c[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t HW = P.H * P.W;
  const uint32_t i = blockIdx.x * kSegBlock + threadIdx.x;
  const size_t base = (size_t)blockIdx.y * HW;
  uint32_t cls = 0xFFu, label = kSegNoLabel, size = 0;
  bool root_accepted = false, root_rejected = false;
  if (i < HW) {
    cls = ws.cls[base + i];
    if (cls == kSegNode) {
      label = ws.root[base + i];
      size = ws.size[base + label];
      const bool acc = seg_accepted(size, ws.line_max[base + label] - label / P.W + 1u, P);
      cls = acc ? kSegCluster : kSegOutlier;
      root_accepted = label == i && acc, root_rejected = label == i && !acc;
    }
    if (out.classes) out.classes[base + i] = (uint8_t)cls;
    if (out.labels) out.labels[base + i] = label;
    if (out.sizes) out.sizes[base + i] = size;
    if (out.filtered) {
      const bool keep = cls == kSegCluster || (cls == kSegOutlier && !P.drop_outliers) || (cls == kSegGround && !P.drop_ground);
      const T* p = scans + (base + i) * 3;
      T v0 = (T)0, v1 = (T)0, v2 = (T)0;
      if (keep) v0 = p[0], v1 = p[1], v2 = p[2];
      T* o = static_cast<T*>(out.filtered) + (base + i) * 3;
      o[0] = v0, o[1] = v1, o[2] = v2;
    }
  }
  seg_count(s_c + 0, cls == kSegInvalid);
  seg_count(s_c + 1, cls == kSegGround);
  seg_count(s_c + 2, cls == kSegCluster);
  seg_count(s_c + 3, cls == kSegOutlier);
  seg_count(s_c + 4, root_accepted);
  seg_count(s_c + 5, root_rejected);
  if (root_accepted || root_rejected) atomicMax(s_c + 6, size);
  __syncthreads();
  uint32_t* stats = ws.stats + (size_t)blockIdx.y * kSegStatWords;
  if (threadIdx.x < 6 && s_c[threadIdx.x]) atomicAdd(stats + threadIdx.x, s_c[threadIdx.x]);
  if (threadIdx.x == 6 && s_c[6]) atomicMax(stats + 6, s_c[6]);
  if (threadIdx.x == 0) ws.block_cnt[(size_t)blockIdx.y * nb + blockIdx.x] = s_c[4];
}

// blockIdx.x = scan
__global__ __launch_bounds__(kSegBlock) void segment_finish_kernel(SegScratch ws, SegOutputs out, uint32_t nb) {
  __shared__ uint32_t s_wave[4];
  const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
  if (out.clusters) {
    uint32_t* cnt = ws.block_cnt + (size_t)blockIdx.x * nb;
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < nb; b0 += kSegBlock) {
      const uint32_t j = b0 + t;
      const uint32_t v = j < nb ? cnt[j] : 0u;
      uint32_t incl = v;
      for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
      }
      if (lane == 63u) s_wave[w] = incl;
      __syncthreads();
      uint32_t before = 0, total = 0;
      for (uint32_t k = 0; k < 4; k++) before += k < w ? s_wave[k] : 0u, total += s_wave[k];
      if (j < nb) cnt[j] = carry + before + incl - v;
      carry += total;
      __syncthreads();
    }
  }
  if (t == 0 && out.stats) {
    const uint32_t* st = ws.stats + (size_t)blockIdx.x * kSegStatWords;
    uint32_t* o = out.stats + (size_t)blockIdx.x * kSegStatWords;
    for (uint32_t k = 0; k < 7; k++) o[k] = st[k];
    o[7] = out.clusters ? (uint32_t)(st[4] < out.max_clusters ? st[4] : out.max_clusters) : 0u;
  }
}

__global__ __launch_bounds__(kSegBlock) void segment_clusters_kernel(SegParams P, SegScratch ws, SegOutputs out, uint32_t nb) {
  __shared__ uint32_t s_wave[4];
  const uint32_t HW = P.H * P.W;
  const uint32_t i = blockIdx.x * kSegBlock + threadIdx.x;
  const size_t base = (size_t)blockIdx.y * HW;
  bool flag = false;
  uint32_t size = 0, line_max = 0;
  if (i < HW && ws.root[base + i] == i) {
    size = ws.size[base + i], line_max = ws.line_max[base + i];
    flag = seg_accepted(size, line_max - i / P.W + 1u, P);
  }
  uint32_t total;
  const uint32_t rank = block_rank(flag, s_wave, total);
  if (flag) {
    const size_t pos = (size_t)ws.block_cnt[(size_t)blockIdx.y * nb + blockIdx.x] + rank;
    if (pos < out.max_clusters) out.clusters[(size_t)blockIdx.y * out.max_clusters + pos] = loamx_segment_cluster{i, size, i / P.W, line_max};
  }
}

template <typename T>
void launch_segment_t(const T* scans, uint32_t n_scans, const SegParams& P, bool tiles, const SegScratch& ws, const SegOutputs& out, hipStream_t s) {
  const uint32_t HW = P.H * P.W, nb = (HW + kSegBlock - 1) / kSegBlock;
  const uint32_t tile_cols = (P.W + TC - 1) / TC, tile_rows = (P.H + TL - 1) / TL;
  const dim3 cells(nb, n_scans), tile_grid(tile_rows * tile_cols, n_scans), block(kSegBlock);
  launch_kernel((segment_classify_kernel<T>), cells, block, 0, s, scans, P, ws);
  if (tiles) launch_kernel((segment_edges_kernel<T, true>), tile_grid, dim3(TC), 0, s, scans, P, ws, tile_cols);
  else launch_kernel((segment_edges_kernel<T, false>), tile_grid, dim3(TC), 0, s, scans, P, ws, tile_cols);
  launch_kernel(segment_merge_kernel, cells, block, 0, s, P, ws);
  launch_kernel(segment_flatten_kernel, cells, block, 0, s, P, ws);
  launch_kernel((segment_decide_kernel<T>), cells, block, 0, s, scans, P, ws, out, nb);
  if (out.clusters || out.stats) launch_kernel(segment_finish_kernel, dim3(n_scans), block, 0, s, ws, out, nb);
  if (out.clusters && out.max_clusters) launch_kernel(segment_clusters_kernel, cells, block, 0, s, P, ws, out, nb);
}

}  // namespace

void launch_segment(const void* d_scans, bool f32, uint32_t n_scans, const SegParams& P, bool tiles, const SegScratch& ws, const SegOutputs& out,
                    hipStream_t s) {
  if (n_scans == 0 || P.H == 0 || P.W == 0) return;
  if (f32) launch_segment_t(static_cast<const float*>(d_scans), n_scans, P, tiles, ws, out, s);
  else launch_segment_t(static_cast<const double*>(d_scans), n_scans, P, tiles, ws, out, s);
}

}  // namespace loamx
