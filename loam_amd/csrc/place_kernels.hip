// place_kernels.hip — scan descriptors and the loop-candidate search (loamx.h, "place recognition"; the arithmetic: place_math.h).
//   build      blockIdx.y = cloud, blockIdx.x = a share of kPlaceBlockPoints of its points. The S sector boundaries (16 B each,
//              at most 5.6 KB) are staged in LDS: every point's bisection reads log2 S of them. Each point is classified and its
//              code raised with an integer atomicMax — in an LDS table of R S words where that fits 48 KB beside the boundaries
//              (R S <= 10 800: the default 20 x 60 is 4.7 KB), whose non-zero cells then go to the cloud's table in the workspace
//              with one global atomicMax each; straight in the cloud's table for the larger shapes. A maximum of integers does not
//              depend on the order of arrival, so neither the split of a cloud over workgroups nor the batch shows in the bytes.
//   finish     narrows the tables to uint16.
//   keys       one workgroup per descriptor: ring sums and squared column norms (add, and the queries of a search).
//   select     the key stage. A workgroup holds kPlaceSelectChunk (key distance, id) records in LDS — the first pass forms them
//              from the stored ring keys, the later passes read the lists the pass before left — ranks each by counting the
//              records ahead of it in (key distance, position) order, and writes those of rank < K at their rank. Position
//              order is id order among equal distances: the chunks cover ascending id ranges and each list is ascending. The
//              passes repeat until one list per query is left; no n_queries x N array of distances exists at any time.
//   shift      one workgroup per (query, candidate): both descriptors and norms in LDS (the entry's stays in global memory
//              where the two together exceed 60 KB: 64 x 360), one thread per (shift, column) pair forms the exact dot
//              product and the quantised cosine and adds it, with the count of columns, to its shift's word by one LDS integer
//              atomic; thread 0 walks the S shifts for the minimum (lowest shift on a tie).
//   order      one workgroup per query ranks the K records by (distance, id).
// Algorithmic bytes — build: 3 scalars per point read, R S x (4 B reset + 4 B read + 2 B written) per cloud; select, first pass:
// 4 R B per (query, entry), 16 K B written per (query, chunk); shift: 2 x (2 R S + 8 S) B read per pair, 24 B written.
#include <string.h>

#include "loamx_internal.h"

namespace loamx {
namespace {

constexpr int kPlaceThreads = 256;
constexpr uint32_t kPlaceBlockPoints = 2048;        // points of a cloud per workgroup of the build
constexpr uint32_t kPlaceLdsBudget = 48u * 1024u;   // LDS table + staged boundaries of the build
constexpr uint32_t kPlaceShiftLds = 60u * 1024u;    // both descriptors + norms + shift words of the shift stage
constexpr int kSelectThreads = 1024;                // the selection: one record per thread
constexpr uint32_t kSelectPerThread = kPlaceSelectChunk / kSelectThreads;

template <typename T, bool kLds>
__global__ __launch_bounds__(kPlaceThreads) void place_build_kernel(const T* __restrict__ pts, uint32_t stride, OrgOffsets offs, PlaceShape P,
                                                                     const double* __restrict__ dirs, uint32_t* __restrict__ table) {
  extern __shared__ __align__(16) unsigned char smem[];
  const uint32_t c = blockIdx.y;
  const unsigned long long first = offs.off[c], n = offs.off[c + 1] - first;
  const unsigned long long b0 = (unsigned long long)blockIdx.x * kPlaceBlockPoints;
  if (b0 >= n) return;  // (the grid covers the largest cloud of the chunk)
  const uint32_t RS = P.R * P.S;
  double* sdirs = reinterpret_cast<double*>(smem);
  uint32_t* cells = reinterpret_cast<uint32_t*>(sdirs + 2 * P.S);
  for (uint32_t i = threadIdx.x; i < 2 * P.S; i += kPlaceThreads) sdirs[i] = dirs[i];
  if (kLds)
    for (uint32_t i = threadIdx.x; i < RS; i += kPlaceThreads) cells[i] = 0u;
  __syncthreads();
  uint32_t* tab = table + (size_t)c * RS;
  const unsigned long long end = n - b0 < kPlaceBlockPoints ? n : b0 + kPlaceBlockPoints;
  for (unsigned long long i = b0 + threadIdx.x; i < end; i += kPlaceThreads) {
    const T* p = pts + (size_t)(first + i) * stride;
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    uint32_t code = 0;
    const uint32_t cell = place_cell(P, sdirs, x, y, z, code);
    if (cell < RS) {  // (kPlaceNoCell is not)
      if (kLds) atomicMax(cells + cell, code);
      else atomicMax(tab + cell, code);
    }
  }
  if (kLds) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < RS; i += kPlaceThreads) {
      const uint32_t v = cells[i];
      if (v) atomicMax(tab + i, v);
    }
  }
}

__global__ __launch_bounds__(kPlaceThreads) void place_finish_kernel(const uint32_t* __restrict__ table, size_t n, uint16_t* __restrict__ desc) {
  const size_t i = (size_t)blockIdx.x * kPlaceThreads + threadIdx.x;
  if (i < n) desc[i] = (uint16_t)table[i];
}

// blockIdx.x = descriptor
__global__ __launch_bounds__(kPlaceThreads) void place_keys_kernel(const uint16_t* __restrict__ desc, uint32_t R, uint32_t S, uint32_t* __restrict__ keys,
                                                                    unsigned long long* __restrict__ norms) {
  const size_t e = blockIdx.x;
  const uint16_t* d = desc + e * R * S;
  for (uint32_t r = threadIdx.x; r < R; r += kPlaceThreads) {
    uint32_t sum = 0;
    for (uint32_t j = 0; j < S; j++) sum += d[r * S + j];
    keys[e * R + r] = sum;
  }
  for (uint32_t j = threadIdx.x; j < S; j += kPlaceThreads) {
    unsigned long long sum = 0;
    for (uint32_t r = 0; r < R; r++) {
      const uint32_t v = d[r * S + j];
      sum += (unsigned long long)(v * v);  // (65535^2 < 2^32)
    }
    norms[e * S + j] = sum;
  }
}

// blockIdx.y = query, blockIdx.x = chunk of kPlaceSelectChunk records; out: [query][chunk][K]. 1 024 threads, one
// record each: a wavefront walks all kPlaceSelectChunk records whatever it owns, its time grows with the records per thread,
// and a search of few queries (most of the device idle) waits for exactly that: four records per thread took four times as
// long per pass there and no less in a full device.
template <bool kFromKeys>
__global__ __launch_bounds__(kSelectThreads) void place_select_kernel(const uint32_t* __restrict__ keys, uint32_t n_entries, uint32_t R,
                                                                      const uint32_t* __restrict__ qkeys, PlaceIdEnd id_end,
                                                                      const PlaceCand* __restrict__ in, uint32_t in_len, PlaceCand* __restrict__ out,
                                                                      uint32_t K) {
  __shared__ unsigned long long sd[kPlaceSelectChunk];
  __shared__ uint32_t sid[kPlaceSelectChunk];
  __shared__ uint32_t qk[kPlaceMaxRings];
  const uint32_t q = blockIdx.y, chunk = blockIdx.x;
  uint32_t limit = in_len;
  if (kFromKeys) {
    if (threadIdx.x < R) qk[threadIdx.x] = qkeys[(size_t)q * R + threadIdx.x];
    limit = n_entries;
    if (id_end.given) {  // (then the launch holds at most kPlaceIdEndQueries queries)
      const uint32_t e = id_end.v[q];
      limit = e < limit ? e : limit;
    }
    __syncthreads();
  }
  unsigned long long mine[kSelectPerThread];
  for (uint32_t t = 0; t < kSelectPerThread; t++) {
    const uint32_t i = threadIdx.x + t * kSelectThreads;
    const uint32_t g = chunk * kPlaceSelectChunk + i;
    unsigned long long dist = kPlaceNoKeyDist;
    uint32_t id = kPlaceNoId;
    if (g < limit) {
      if (kFromKeys) {
        const uint32_t* k = keys + (size_t)g * R;
        dist = 0;
        for (uint32_t r = 0; r < R; r++) {
          const long long diff = (long long)qk[r] - (long long)k[r];
          dist += (unsigned long long)(diff * diff);
        }
        id = g;
      } else {
        const PlaceCand rec = in[(size_t)q * in_len + g];
        dist = rec.dist, id = rec.id;
      }
    }
    sd[i] = dist, sid[i] = id, mine[t] = dist;
  }
  __syncthreads();
  uint32_t rank[kSelectPerThread];
  for (uint32_t t = 0; t < kSelectPerThread; t++) rank[t] = 0;
  for (uint32_t j = 0; j < kPlaceSelectChunk; j++) {
    const unsigned long long dj = sd[j];
    for (uint32_t t = 0; t < kSelectPerThread; t++) {
      const uint32_t i = threadIdx.x + t * kSelectThreads;
      rank[t] += (dj < mine[t] || (dj == mine[t] && j < i)) ? 1u : 0u;
    }
  }
  PlaceCand* o = out + ((size_t)q * gridDim.x + chunk) * K;
  for (uint32_t t = 0; t < kSelectPerThread; t++)
    if (rank[t] < K) o[rank[t]] = PlaceCand{mine[t], sid[threadIdx.x + t * kSelectThreads], 0u};
}

// blockIdx.y = query, blockIdx.x = candidate slot. LDS: [S] shift words, [S] query norms, [S] entry norms, the query's
// descriptor, the entry's (kEntryLds).
template <bool kEntryLds>
__global__ __launch_bounds__(kPlaceThreads) void place_shift_kernel(PlaceEntries E, uint32_t R, uint32_t S, const uint16_t* __restrict__ qdesc,
                                                                     const unsigned long long* __restrict__ qnorms, const PlaceCand* __restrict__ cands,
                                                                     uint32_t K, loamx_place_match* __restrict__ out) {
  extern __shared__ __align__(16) unsigned char smem[];
  const uint32_t q = blockIdx.y, slot = blockIdx.x, RS = R * S;
  const PlaceCand cand = cands[(size_t)q * K + slot];
  loamx_place_match* rec = out + (size_t)q * K + slot;
  if (cand.id >= E.n) {  // (kPlaceNoId: fewer than K eligible entries)
    if (threadIdx.x == 0) rec->id = kPlaceNoId, rec->shift = 0u, rec->key_dist = kPlaceNoKeyDist, rec->distance = 2.0;
    return;
  }
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem);  // m << 40 | score (score <= 360 x 2^30 < 2^39)
  unsigned long long* nq = acc + S;
  unsigned long long* ne = nq + S;
  uint16_t* dq = reinterpret_cast<uint16_t*>(ne + S);
  uint16_t* de_lds = dq + RS;
  const uint16_t* de_glob = E.desc + (size_t)cand.id * RS;
  for (uint32_t i = threadIdx.x; i < S; i += kPlaceThreads) {
    acc[i] = 0ull, nq[i] = qnorms[(size_t)q * S + i], ne[i] = E.norms[(size_t)cand.id * S + i];
  }
  for (uint32_t i = threadIdx.x; i < RS; i += kPlaceThreads) {
    dq[i] = qdesc[(size_t)q * RS + i];
    if (kEntryLds) de_lds[i] = de_glob[i];
  }
  __syncthreads();
  const uint16_t* de = kEntryLds ? de_lds : de_glob;
  for (uint32_t t = threadIdx.x; t < S * S; t += kPlaceThreads) {
    const uint32_t s = t / S, j = t - s * S;
    const uint32_t jj = j + s >= S ? j + s - S : j + s;
    const unsigned long long a = nq[j], b = ne[jj];
    if (a == 0ull || b == 0ull) continue;
    unsigned long long dot = 0;
    for (uint32_t r = 0; r < R; r++) dot += (unsigned long long)((uint32_t)dq[r * S + j] * (uint32_t)de[r * S + jj]);
    atomicAdd(acc + s, (1ull << 40) | place_cos_q(dot, a, b));
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double best = 0.0;
    uint32_t best_s = 0;
    for (uint32_t s = 0; s < S; s++) {
      const unsigned long long w = acc[s];
      const double d = place_shift_distance(w & ((1ull << 40) - 1), (uint32_t)(w >> 40));
      if (s == 0 || d < best) best = d, best_s = s;
    }
    rec->id = cand.id, rec->shift = best_s, rec->key_dist = cand.dist, rec->distance = best;
  }
}

// blockIdx.x = query: its K records ascending by (distance, id); equal pairs (the records without an entry) by slot
__global__ __launch_bounds__(kPlaceMaxCandidates) void place_order_kernel(const loamx_place_match* __restrict__ in, uint32_t K,
                                                                           loamx_place_match* __restrict__ out) {
  __shared__ loamx_place_match rec[kPlaceMaxCandidates];
  const uint32_t i = threadIdx.x;
  if (i < K) rec[i] = in[(size_t)blockIdx.x * K + i];
  __syncthreads();
  if (i >= K) return;
  const loamx_place_match me = rec[i];
  uint32_t rank = 0;
  for (uint32_t j = 0; j < K; j++) {
    const loamx_place_match o = rec[j];
    const bool ahead = o.distance < me.distance || (o.distance == me.distance && (o.id < me.id || (o.id == me.id && j < i)));
    rank += ahead ? 1u : 0u;
  }
  out[(size_t)blockIdx.x * K + rank] = me;
}

template <typename T>
void launch_build_t(const T* pts, uint32_t stride, const OrgOffsets& offs, uint32_t n_clouds, unsigned long long max_points, const PlaceShape& P,
                    const double* d_dirs, uint32_t* table, hipStream_t s) {
  const uint32_t RS = P.R * P.S;
  const size_t dirs_bytes = (size_t)P.S * 2 * sizeof(double), lds_bytes = dirs_bytes + (size_t)RS * sizeof(uint32_t);
  const dim3 grid((unsigned)((max_points + kPlaceBlockPoints - 1) / kPlaceBlockPoints), n_clouds), block(kPlaceThreads);
  if (lds_bytes <= kPlaceLdsBudget) launch_kernel((place_build_kernel<T, true>), grid, block, lds_bytes, s, pts, stride, offs, P, d_dirs, table);
  else launch_kernel((place_build_kernel<T, false>), grid, block, dirs_bytes, s, pts, stride, offs, P, d_dirs, table);
}

}  // namespace

void launch_place_descriptors(const void* d_points, bool f32, uint32_t stride, const OrgOffsets& offs, uint32_t n_clouds,
                              unsigned long long max_points, const PlaceShape& P, const double* d_dirs, uint32_t* table, uint16_t* d_desc,
                              hipStream_t s) {
  if (n_clouds == 0) return;
  if (max_points > 0) {
    if (f32) launch_build_t(static_cast<const float*>(d_points), stride, offs, n_clouds, max_points, P, d_dirs, table, s);
    else launch_build_t(static_cast<const double*>(d_points), stride, offs, n_clouds, max_points, P, d_dirs, table, s);
  }
  const size_t n = (size_t)n_clouds * P.R * P.S;
  launch_kernel(place_finish_kernel, dim3((unsigned)((n + kPlaceThreads - 1) / kPlaceThreads)), dim3(kPlaceThreads), 0, s, (const uint32_t*)table, n,
                d_desc);
}

void launch_place_keys(const uint16_t* d_desc, size_t n, const PlaceShape& P, uint32_t* d_keys, unsigned long long* d_norms, hipStream_t s) {
  if (n == 0) return;
  launch_kernel(place_keys_kernel, dim3((unsigned)n), dim3(kPlaceThreads), 0, s, d_desc, P.R, P.S, d_keys, d_norms);
}

uint32_t place_select_chunks(uint32_t n_entries) {
  const uint32_t c = (n_entries + kPlaceSelectChunk - 1) / kPlaceSelectChunk;
  return c ? c : 1u;
}
size_t place_select_records(uint32_t n_entries, uint32_t K) { return (size_t)place_select_chunks(n_entries) * K; }

PlaceCand* launch_place_key_stage(const PlaceEntries& E, const PlaceShape& P, const uint32_t* d_qkeys, const uint32_t* id_end, uint32_t n_queries,
                                  uint32_t K, PlaceCand* buf_a, PlaceCand* buf_b, hipStream_t s) {
  uint32_t chunks = place_select_chunks(E.n);
  PlaceIdEnd ends;
  memset(&ends, 0, sizeof(ends));
  if (id_end) {
    ends.given = 1u;
    for (uint32_t q = 0; q < n_queries && q < kPlaceIdEndQueries; q++) ends.v[q] = id_end[q];
  }
  launch_kernel((place_select_kernel<true>), dim3(chunks, n_queries), dim3(kSelectThreads), 0, s, E.keys, E.n, P.R, d_qkeys, ends,
                (const PlaceCand*)nullptr, 0u, buf_a, K);
  ends.given = 0u;
  PlaceCand *from = buf_a, *to = buf_b;
  while (chunks > 1) {
    const uint32_t len = chunks * K;
    chunks = place_select_chunks(len);
    launch_kernel((place_select_kernel<false>), dim3(chunks, n_queries), dim3(kSelectThreads), 0, s, (const uint32_t*)nullptr, 0u, 0u,
                  (const uint32_t*)nullptr, ends, (const PlaceCand*)from, len, to, K);
    PlaceCand* t = from;
    from = to, to = t;
  }
  return from;
}

void launch_place_shift_stage(const PlaceEntries& E, const PlaceShape& P, const uint16_t* d_qdesc, const unsigned long long* d_qnorms,
                              const PlaceCand* cands, uint32_t n_queries, uint32_t K, loamx_place_match* d_tmp, loamx_place_match* d_out,
                              hipStream_t s) {
  const size_t RS = (size_t)P.R * P.S, base = (size_t)P.S * 3 * sizeof(unsigned long long);
  const dim3 grid(K, n_queries), block(kPlaceThreads);
  if (base + 2 * RS * sizeof(uint16_t) <= kPlaceShiftLds)
    launch_kernel((place_shift_kernel<true>), grid, block, base + 2 * RS * sizeof(uint16_t), s, E, P.R, P.S, d_qdesc, d_qnorms, cands, K, d_tmp);
  else
    launch_kernel((place_shift_kernel<false>), grid, block, base + RS * sizeof(uint16_t), s, E, P.R, P.S, d_qdesc, d_qnorms, cands, K, d_tmp);
  launch_kernel(place_order_kernel, dim3(n_queries), dim3(kPlaceMaxCandidates), 0, s, (const loamx_place_match*)d_tmp, K, d_out);
}

}  // namespace loamx
