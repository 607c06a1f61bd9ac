// posegraph_kernels.hip — the pose-graph optimiser's kernels (loamx.h: "pose graph"; the arithmetic: posegraph_math.h).
//
// One workgroup of kPgoChunk = 256 threads per chunk of 256 poses or edges: a workgroup IS a chunk of the ordered sums, so
// a cross-thread sum is the header's tree over the workgroup's LDS array, one partial per workgroup, and the partials are
// added in ascending order by thread 0 of every workgroup of the kernel that needs the scalar (same order, same bytes in
// every workgroup): a reduction costs no launch. No floating-point atomics; the only atomics are the integer degree
// counts, the fill cursors (whose order the per-pose sort removes) and the bad-edge count.
//
// The state of a solve (PgoState) lives in two device copies: a kernel that changes it reads copy `in`, every workgroup
// derives the same new state, workgroup 0 writes copy `out`. The host enqueues a fixed sequence of launches and never reads
// anything back: once `done` is set every later launch returns at its first branch.
#include "loamx_internal.h"
#include "posegraph_math.h"

namespace loamx {
namespace {

constexpr int kT = (int)kPgoChunk;

// the header's tree over the workgroup's 256 values; the result is in v[0] for every thread after the last barrier
__device__ __forceinline__ void block_tree_add(double* v) {
  __syncthreads();
  for (uint32_t s = kPgoChunk / 2; s > 0; s >>= 1) {
    pgo_tree_add(v, threadIdx.x, s);
    __syncthreads();
  }
}
__device__ __forceinline__ void block_tree_max(double* v) {
  __syncthreads();
  for (uint32_t s = kPgoChunk / 2; s > 0; s >>= 1) {
    pgo_tree_max(v, threadIdx.x, s);
    __syncthreads();
  }
}
// thread 0 adds the partials in chunk order; everybody gets the sum
__device__ __forceinline__ double block_sum_chunks(const double* part, uint32_t n_chunks, double* s_slot) {
  if (threadIdx.x == 0) *s_slot = pgo_sum_chunks(part, n_chunks);
  __syncthreads();
  return *s_slot;
}

__global__ void pgo_init_kernel(PgoParams P, PgoState* st) {
  PgoState s;
  pgo_state_init(s, P);
  st[0] = s;
}

// degree counts (threads over the edges) and the fixed flags as the kernels read them (threads over the poses)
__global__ __launch_bounds__(kT) void pgo_degree_kernel(const PgoEdge* __restrict__ edges, uint32_t n_edges, uint32_t n_poses,
                                                        const uint8_t* __restrict__ d_fixed, uint32_t* deg, uint8_t* fixed, uint32_t* n_bad) {
  const uint32_t t = blockIdx.x * kT + threadIdx.x;
  if (t < n_poses) fixed[t] = d_fixed ? (d_fixed[t] != 0) : (t == 0);
  if (t < n_edges) {
    const uint32_t a = edges[t].a, b = edges[t].b;
    if (pgo_edge_ok(a, b, n_poses)) atomicAdd(&deg[a], 1u), atomicAdd(&deg[b], 1u);
    else atomicAdd(n_bad, 1u);
  }
}

// one workgroup: exclusive scan of the degrees into off[0 .. n_poses], the fill cursors, the count of free poses; then the
// refusal / nothing-to-do decision (the state is written in place: nobody else runs)
__global__ __launch_bounds__(1024) void pgo_scan_kernel(const uint32_t* __restrict__ deg, const uint8_t* __restrict__ fixed, uint32_t n_poses,
                                                        uint32_t n_edges, const uint32_t* __restrict__ n_bad, uint32_t* off, uint32_t* cursor,
                                                        PgoState* st) {
  __shared__ uint32_t s_a[1024], s_b[1024], s_free[1024];
  const uint32_t t = threadIdx.x;
  const uint32_t bad = *n_bad;
  uint32_t carry = 0, n_free = 0;
  if (!bad) {
    for (uint32_t base = 0; base < n_poses; base += 1024) {
      const uint32_t i = base + t;
      const uint32_t d = i < n_poses ? deg[i] : 0u;
      n_free += (i < n_poses && !fixed[i]) ? 1u : 0u;
      uint32_t *cur = s_a, *nxt = s_b;
      cur[t] = d;
      __syncthreads();
      for (uint32_t s = 1; s < 1024; s <<= 1) {
        nxt[t] = t >= s ? cur[t] + cur[t - s] : cur[t];
        __syncthreads();
        uint32_t* tmp = cur;
        cur = nxt, nxt = tmp;
      }
      const uint32_t incl = cur[t], total = cur[1023];
      if (i < n_poses) off[i] = carry + incl - d, cursor[i] = carry + incl - d;
      carry += total;
      __syncthreads();
    }
    if (t == 0) off[n_poses] = carry;
  }
  s_free[t] = n_free;
  __syncthreads();
  for (uint32_t s = 512; s > 0; s >>= 1) {
    if (t < s) s_free[t] += s_free[t + s];
    __syncthreads();
  }
  if (t == 0) {
    PgoState s = st[0];
    pgo_state_counts(s, bad, n_edges, s_free[0]);
    st[0] = s;
  }
}

__global__ __launch_bounds__(kT) void pgo_fill_kernel(const PgoEdge* __restrict__ edges, uint32_t n_edges, uint32_t* cursor, uint32_t* list,
                                                      const PgoState* __restrict__ st) {
  if (st->done) return;
  const uint32_t e = blockIdx.x * kT + threadIdx.x;
  if (e >= n_edges) return;
  list[atomicAdd(&cursor[edges[e].a], 1u)] = 2u * e;
  list[atomicAdd(&cursor[edges[e].b], 1u)] = 2u * e + 1u;
}

__global__ __launch_bounds__(kT) void pgo_sort_kernel(const uint32_t* __restrict__ off, uint32_t n_poses, uint32_t* list,
                                                      const PgoState* __restrict__ st) {
  if (st->done) return;
  const uint32_t i = blockIdx.x * kT + threadIdx.x;
  if (i >= n_poses) return;
  pgo_sort_segment(list + off[i], off[i + 1] - off[i]);
}

// Per edge at `poses`: kFull: the blocks (and the read-out record when lin != nullptr); always the edge's cost into the
// chunk partial cost_part[workgroup]. ignore_done: the read-out entry point runs it outside a solve.
template <bool kFull>
__global__ __launch_bounds__(kT) void pgo_linearize_kernel(const double* __restrict__ poses, const PgoEdge* __restrict__ edges, uint32_t n_edges,
                                                           double huber_delta, PgoLinearization* lin, PgoEdgeBlocks* blocks, double* cost_part,
                                                           const PgoState* __restrict__ st, uint32_t ignore_done) {
  __shared__ double s_v[kT];
  if (!ignore_done && st->done) return;
  const uint32_t e = blockIdx.x * kT + threadIdx.x;
  double cost = 0.0;
  if (e < n_edges) {
    const PgoEdge& ed = edges[e];
    double Ta[7], Tb[7];
#pragma unroll
    for (int k = 0; k < 7; k++) Ta[k] = poses[7 * (size_t)ed.a + k], Tb[k] = poses[7 * (size_t)ed.b + k];
    if (kFull) cost = pgo_linearize_edge(Ta, Tb, ed, huber_delta, lin ? lin + e : nullptr, blocks ? blocks + e : nullptr);
    else cost = pgo_edge_cost(Ta, Tb, ed, huber_delta);
  }
  s_v[threadIdx.x] = cost;
  block_tree_add(s_v);
  if (threadIdx.x == 0) cost_part[blockIdx.x] = s_v[0];
}

struct PgoVectors {
  double *x, *r, *z, *q, *p[2];
};

__global__ __launch_bounds__(kT) void pgo_gather_kernel(uint32_t n_poses, const uint8_t* __restrict__ fixed, const uint32_t* __restrict__ off,
                                                        const uint32_t* __restrict__ list, const PgoEdgeBlocks* __restrict__ blocks,
                                                        const double* __restrict__ cost_part, uint32_t n_edge_chunks, PgoPoseBlocks* pose_blocks,
                                                        PgoVectors V, double* rz_part, const PgoState* __restrict__ in, PgoState* out) {
  __shared__ double s_v[kT];
  __shared__ double s_slot;
  PgoState s = *in;
  if (s.done) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = s;
    return;
  }
  pgo_state_gather(s, block_sum_chunks(cost_part, n_edge_chunks, &s_slot));
  const uint32_t i = blockIdx.x * kT + threadIdx.x;
  double rz = 0.0;
  if (i < n_poses) {
    double x[6], r[6], z[6];
    rz = pgo_gather_pose(fixed[i] != 0, list + off[i], off[i + 1] - off[i], blocks, s.lambda, pose_blocks[i], x, r, z);
#pragma unroll
    for (int k = 0; k < 6; k++) V.x[6 * (size_t)i + k] = x[k], V.r[6 * (size_t)i + k] = r[k], V.z[6 * (size_t)i + k] = z[k];
  }
  s_v[threadIdx.x] = rz;
  block_tree_add(s_v);
  if (threadIdx.x == 0) rz_part[blockIdx.x] = s_v[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) *out = s;
}

// PCG iteration, first launch: beta from the r.z partials, the direction, q = (H + damping) p, the p.q partials
__global__ __launch_bounds__(kT) void pgo_spmv_kernel(uint32_t n_poses, uint32_t n_pose_chunks, const uint8_t* __restrict__ fixed,
                                                      const uint32_t* __restrict__ off, const uint32_t* __restrict__ list,
                                                      const PgoEdge* __restrict__ edges, const PgoEdgeBlocks* __restrict__ blocks,
                                                      const PgoPoseBlocks* __restrict__ pose_blocks, PgoVectors V, uint32_t p_in,
                                                      const double* __restrict__ rz_part, double* pq_part, double pcg_tolerance,
                                                      const PgoState* __restrict__ in, PgoState* out) {
  __shared__ double s_v[kT];
  __shared__ double s_slot;
  PgoState s = *in;
  if (s.done || s.pcg_done) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = s;
    return;
  }
  const bool first = s.pcg_it == 0;
  pgo_state_spmv(s, block_sum_chunks(rz_part, n_pose_chunks, &s_slot), pcg_tolerance);
  if (s.pcg_done) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = s;
    return;
  }
  const uint32_t i = blockIdx.x * kT + threadIdx.x;
  double pq = 0.0;
  if (i < n_poses) {
    const PgoPoseBlocks& pb = pose_blocks[i];
    const bool dead = pgo_pose_dead(fixed[i] != 0, pb);
    pq =pgo_spmv_row(i, dead, fixed, list + off[i], off[i + 1] - off[i], edges, blocks, pb, V.z, V.p[p_in], first, s.beta, V.p[p_in ^ 1u], V.q);
  }
  s_v[threadIdx.x] = pq;
  block_tree_add(s_v);
  if (threadIdx.x == 0) pq_part[blockIdx.x] = s_v[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) *out = s;
}

// PCG iteration, second launch: alpha from the p.q partials, x, r, z, the r.z partials
__global__ __launch_bounds__(kT) void pgo_update_kernel(uint32_t n_poses, uint32_t n_pose_chunks, const PgoPoseBlocks* __restrict__ pose_blocks,
                                                        PgoVectors V, uint32_t p_cur, const double* __restrict__ pq_part, double* rz_part,
                                                        uint32_t pcg_cap, const PgoState* __restrict__ in, PgoState* out) {
  __shared__ double s_v[kT];
  __shared__ double s_slot;
  PgoState s = *in;
  if (s.done || s.pcg_done) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = s;
    return;
  }
  pgo_state_update(s, block_sum_chunks(pq_part, n_pose_chunks, &s_slot), pcg_cap);
  if (s.pcg_done == 1) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = s;
    return;
  }
  const uint32_t i = blockIdx.x * kT + threadIdx.x;
  double rz = 0.0;
  if (i < n_poses) rz = pgo_update_pose(i, pose_blocks[i], s.alpha, V.p[p_cur], V.q, V.x, V.r, V.z);
  s_v[threadIdx.x] = rz;
  block_tree_add(s_v);
  if (threadIdx.x == 0) rz_part[blockIdx.x] = s_v[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) *out = s;
}

__global__ __launch_bounds__(kT) void pgo_candidate_kernel(uint32_t n_poses, const uint8_t* __restrict__ fixed, const double* __restrict__ poses,
                                                           const double* __restrict__ x, double* cand, double* max_part,
                                                           const PgoState* __restrict__ st) {
  __shared__ double s_v[kT];
  if (st->done) return;
  const uint32_t i = blockIdx.x * kT + threadIdx.x;
  double m = 0.0;
  if (i < n_poses) {
    double T[7], d[6], o[7];
#pragma unroll
    for (int k = 0; k < 7; k++) T[k] = poses[7 * (size_t)i + k];
#pragma unroll
    for (int k = 0; k < 6; k++) d[k] = x[6 * (size_t)i + k];
    m = pgo_retract(fixed[i] != 0, T, d, o);
#pragma unroll
    for (int k = 0; k < 7; k++) cand[7 * (size_t)i + k] = o[k];
  }
  s_v[threadIdx.x] = m;
  block_tree_max(s_v);
  if (threadIdx.x == 0) max_part[blockIdx.x] = s_v[0];
}

// accept / reject / lambda / termination from the candidate's cost partials and the max |delta| partials; an accepted
// candidate becomes the poses
__global__ __launch_bounds__(kT) void pgo_decide_kernel(uint32_t n_poses, uint32_t n_pose_chunks, uint32_t n_edge_chunks, PgoParams P,
                                                        const double* __restrict__ cand, double* poses, const double* __restrict__ cost_part,
                                                        const double* __restrict__ max_part, const PgoState* __restrict__ in, PgoState* out) {
  __shared__ double s_c1, s_mx;
  PgoState s = *in;
  if (s.done) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = s;
    return;
  }
  if (threadIdx.x == 0) s_c1 = pgo_sum_chunks(cost_part, n_edge_chunks), s_mx = pgo_max_chunks(max_part, n_pose_chunks);
  __syncthreads();
  const bool accept = pgo_state_decide(s, P, s_c1, s_mx);
  const uint32_t i = blockIdx.x * kT + threadIdx.x;
  if (accept && i < n_poses) {
#pragma unroll
    for (int k = 0; k < 7; k++) poses[7 * (size_t)i + k] = cand[7 * (size_t)i + k];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *out = s;
}

__global__ void pgo_nothing_kernel(PgoParams P, PgoSummary* out) {
  PgoState s;
  PgoSummary r;
  pgo_state_init(s, P);
  pgo_state_counts(s, 0u, 0u, 0u);
  pgo_state_summary(s, r);
  *out = r;
}

__global__ void pgo_summary_kernel(const PgoState* __restrict__ st, PgoSummary* out) {
  PgoSummary r;
  pgo_state_summary(*st, r);
  *out = r;
}

// the odometry edges of a sequence: pair p -> (first_id + p, first_id + p + 1, results[p].pose, info[p].information)
__global__ __launch_bounds__(kT) void pgo_edges_from_results_kernel(const loamx_reg_result* __restrict__ results,
                                                                    const loamx_reg_information* __restrict__ info, uint32_t n_pairs,
                                                                    uint32_t first_id, PgoEdge* edges) {
  const uint32_t p = blockIdx.x * kT + threadIdx.x;
  if (p >= n_pairs) return;
  PgoEdge& e = edges[p];
  e.a = first_id + p, e.b = first_id + p + 1u;
  for (int k = 0; k < 7; k++) e.z[k] = results[p].pose[k];
  for (int k = 0; k < 36; k++) e.info[k] = info[p].information[k];
}

inline uint32_t chunks_of(size_t n) { return (uint32_t)((n + kPgoChunk - 1) / kPgoChunk); }

}  // namespace

PgoLayout pgo_layout(size_t n_poses, size_t n_edges) {
  PgoLayout L = {};
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += align256(bytes);
    return at;
  };
  const size_t pc = chunks_of(n_poses), ec = chunks_of(n_edges);
  L.state = take(2 * sizeof(PgoState));
  L.zeroed = take((n_poses + 1) * sizeof(uint32_t));  // n_bad, then deg[n_poses]
  L.zeroed_bytes = (n_poses + 1) * sizeof(uint32_t);
  L.off = take((n_poses + 1) * sizeof(uint32_t));
  L.cursor = take(n_poses * sizeof(uint32_t));
  L.list = take(2 * n_edges * sizeof(uint32_t));
  L.fixed = take(n_poses);
  L.blocks = take(n_edges * sizeof(PgoEdgeBlocks));
  L.pose_blocks = take(n_poses * sizeof(PgoPoseBlocks));
  for (int k = 0; k < 6; k++) L.vec[k] = take(n_poses * 6 * sizeof(double));
  L.cand = take(n_poses * 7 * sizeof(double));
  L.cost_part = take(ec * sizeof(double));
  L.cand_cost_part = take(ec * sizeof(double));
  L.rz_part = take(pc * sizeof(double));
  L.pq_part = take(pc * sizeof(double));
  L.max_part = take(pc * sizeof(double));
  L.bytes = o;
  return L;
}

size_t pgo_readout_ws_bytes(size_t n_edges) { return (size_t)chunks_of(n_edges) * sizeof(double); }

// the solver's linearisation kernel with the read-out records in place of the blocks (cost_part: pgo_readout_ws_bytes)
void launch_pgo_linearize_readout(const double* d_poses, const loamx_pgo_edge* d_edges, size_t n_edges, double huber_delta,
                                  loamx_pgo_linearization* d_lin, double* cost_part, hipStream_t s) {
  launch_kernel(pgo_linearize_kernel<true>, dim3(chunks_of(n_edges)), dim3(kT), 0, s, d_poses, reinterpret_cast<const PgoEdge*>(d_edges),
                (uint32_t)n_edges, huber_delta, reinterpret_cast<PgoLinearization*>(d_lin), (PgoEdgeBlocks*)nullptr, cost_part,
                (const PgoState*)nullptr, 1u);
}

static PgoParams pgo_params_of(const loamx_pgo_params& params) {
  PgoParams P;
  P.max_iterations = params.max_iterations, P.max_pcg_iterations = params.max_pcg_iterations, P.pcg_tolerance = params.pcg_tolerance;
  P.initial_lambda = params.initial_lambda, P.cost_tolerance = params.cost_tolerance, P.step_tolerance = params.step_tolerance;
  P.huber_delta = params.huber_delta;
  return P;
}

// a graph without poses or without edges: the summary alone
void launch_pgo_nothing(const loamx_pgo_params& params, loamx_pgo_summary* d_summary, hipStream_t s) {
  if (d_summary) launch_kernel(pgo_nothing_kernel, dim3(1), dim3(1), 0, s, pgo_params_of(params), reinterpret_cast<PgoSummary*>(d_summary));
}

void launch_pgo_solve(double* d_poses, size_t n_poses, const uint8_t* d_fixed, const loamx_pgo_edge* d_edges_c, size_t n_edges,
                      const loamx_pgo_params& params, loamx_pgo_summary* d_summary, void* ws, hipStream_t s) {
  const PgoLayout L = pgo_layout(n_poses, n_edges);
  char* w = static_cast<char*>(ws);
  const PgoParams P = pgo_params_of(params);
  const PgoEdge* edges = reinterpret_cast<const PgoEdge*>(d_edges_c);
  PgoState* st = reinterpret_cast<PgoState*>(w + L.state);
  uint32_t* n_bad = reinterpret_cast<uint32_t*>(w + L.zeroed);
  uint32_t* deg = n_bad + 1;
  uint32_t* off = reinterpret_cast<uint32_t*>(w + L.off);
  uint32_t* cursor = reinterpret_cast<uint32_t*>(w + L.cursor);
  uint32_t* list = reinterpret_cast<uint32_t*>(w + L.list);
  uint8_t* fixed = reinterpret_cast<uint8_t*>(w + L.fixed);
  PgoEdgeBlocks* blocks = reinterpret_cast<PgoEdgeBlocks*>(w + L.blocks);
  PgoPoseBlocks* pose_blocks = reinterpret_cast<PgoPoseBlocks*>(w + L.pose_blocks);
  PgoVectors V;
  V.x = reinterpret_cast<double*>(w + L.vec[0]), V.r = reinterpret_cast<double*>(w + L.vec[1]), V.z = reinterpret_cast<double*>(w + L.vec[2]);
  V.q = reinterpret_cast<double*>(w + L.vec[3]), V.p[0] = reinterpret_cast<double*>(w + L.vec[4]), V.p[1] = reinterpret_cast<double*>(w + L.vec[5]);
  double* cand = reinterpret_cast<double*>(w + L.cand);
  double* cost_part = reinterpret_cast<double*>(w + L.cost_part);
  double* cand_cost_part = reinterpret_cast<double*>(w + L.cand_cost_part);
  double* rz_part = reinterpret_cast<double*>(w + L.rz_part);
  double* pq_part = reinterpret_cast<double*>(w + L.pq_part);
  double* max_part = reinterpret_cast<double*>(w + L.max_part);
  const uint32_t np = (uint32_t)n_poses, ne = (uint32_t)n_edges, pc = chunks_of(n_poses), ec = chunks_of(n_edges);
  const uint32_t both = chunks_of(n_poses > n_edges ? n_poses : n_edges);
  const uint32_t cap = pgo_pcg_cap(P.max_pcg_iterations, n_poses);
  const dim3 T(kT);

  (void)hipMemsetAsync(w + L.zeroed, 0, L.zeroed_bytes, s);
  launch_kernel(pgo_init_kernel, dim3(1), dim3(1), 0, s, P, st);
  launch_kernel(pgo_degree_kernel, dim3(both), T, 0, s, edges, ne, np, d_fixed, deg, fixed, n_bad);
  launch_kernel(pgo_scan_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t*)deg, (const uint8_t*)fixed, np, ne, (const uint32_t*)n_bad, off,
                cursor, st);
  launch_kernel(pgo_fill_kernel, dim3(ec), T, 0, s, edges, ne, cursor, list, (const PgoState*)st);
  launch_kernel(pgo_sort_kernel, dim3(pc), T, 0, s, (const uint32_t*)off, np, list, (const PgoState*)st);
  uint32_t cur = 0;  // the copy of the state that is current
  for (uint32_t it = 0; it < P.max_iterations; it++) {
    launch_kernel(pgo_linearize_kernel<true>, dim3(ec), T, 0, s, (const double*)d_poses, edges, ne, P.huber_delta, (PgoLinearization*)nullptr,
                  blocks, cost_part, (const PgoState*)(st + cur), 0u);
    launch_kernel(pgo_gather_kernel, dim3(pc), T, 0, s, np, (const uint8_t*)fixed, (const uint32_t*)off, (const uint32_t*)list,
                  (const PgoEdgeBlocks*)blocks, (const double*)cost_part, ec, pose_blocks, V, rz_part, (const PgoState*)(st + cur),
                  st + (cur ^ 1u));
    cur ^= 1u;
    // iteration j reads p of V.p[j & 1] (unread when j == 0) and leaves the new direction in the other array
    for (uint32_t j = 0; j < cap; j++) {
      launch_kernel(pgo_spmv_kernel, dim3(pc), T, 0, s, np, pc, (const uint8_t*)fixed, (const uint32_t*)off, (const uint32_t*)list, edges,
                    (const PgoEdgeBlocks*)blocks, (const PgoPoseBlocks*)pose_blocks, V, j & 1u, (const double*)rz_part, pq_part, P.pcg_tolerance,
                    (const PgoState*)(st + cur), st + (cur ^ 1u));
      cur ^= 1u;
      launch_kernel(pgo_update_kernel, dim3(pc), T, 0, s, np, pc, (const PgoPoseBlocks*)pose_blocks, V, (j & 1u) ^ 1u, (const double*)pq_part,
                    rz_part, cap, (const PgoState*)(st + cur), st + (cur ^ 1u));
      cur ^= 1u;
    }
    launch_kernel(pgo_candidate_kernel, dim3(pc), T, 0, s, np, (const uint8_t*)fixed, (const double*)d_poses, (const double*)V.x, cand, max_part,
                  (const PgoState*)(st + cur));
    launch_kernel(pgo_linearize_kernel<false>, dim3(ec), T, 0, s, (const double*)cand, edges, ne, P.huber_delta, (PgoLinearization*)nullptr,
                  (PgoEdgeBlocks*)nullptr, cand_cost_part, (const PgoState*)(st + cur), 0u);
    launch_kernel(pgo_decide_kernel, dim3(pc), T, 0, s, np, pc, ec, P, (const double*)cand, d_poses, (const double*)cand_cost_part,
                  (const double*)max_part, (const PgoState*)(st + cur), st + (cur ^ 1u));
    cur ^= 1u;
  }
  if (d_summary)
    launch_kernel(pgo_summary_kernel, dim3(1), dim3(1), 0, s, (const PgoState*)(st + cur), reinterpret_cast<PgoSummary*>(d_summary));
}

void launch_pgo_edges_from_results(const loamx_reg_result* d_results, const loamx_reg_information* d_info, size_t n_pairs, uint32_t first_id,
                                   loamx_pgo_edge* d_edges, hipStream_t s) {
  if (n_pairs == 0) return;
  launch_kernel(pgo_edges_from_results_kernel, dim3(chunks_of(n_pairs)), dim3(kT), 0, s, d_results, d_info, (uint32_t)n_pairs, first_id,
                reinterpret_cast<PgoEdge*>(d_edges));
}

}  // namespace loamx
