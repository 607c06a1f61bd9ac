// info_kernels.hip — the registration information matrix (loamx.h: loamx_reg_information; arithmetic in info_math.h).
// Two kernels behind one association pass (launch_associate): information_kernel streams the association records of every
// pair and leaves one partial per (pair, chunk); information_finish_kernel adds a pair's partials in chunk order, mirrors the
// triangle, takes the eigenpairs and writes the record. A third, info_activate_kernel, lets the association kernels run once
// more for pairs whose registration has stopped.
#include "loamx_internal.h"
#include "info_math.h"

namespace loamx {

namespace {

static_assert(sizeof(InfoPartial::s) == kInfoSums * sizeof(double), "InfoPartial holds the sums of info_math.h");
static_assert(sizeof(loamx_reg_information) == 696, "loamx.h documents the record's size");

// The slot space of a pair is [edge slots 0..n_se) ++ [plane slots 0..n_sp), as sweep_kernel's; chunk c is slots
// [c * kInfoChunk, (c + 1) * kInfoChunk) of it — a function of the pair alone, whatever the batch and its capacities, so a
// pair's record has the same bytes alone and inside any batch. Thread t of a chunk takes slots t, t + 256, ... in that order.
constexpr int kInfoThreads = 256;
constexpr int kInfoItems = 16;
constexpr int kInfoChunk = kInfoThreads * kInfoItems;

__global__ void info_activate_kernel(RegBatch B) {
  const size_t pair = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pair >= B.n_pairs) return;
  if (pair == 0 && B.live) B.live->stamp[0] = B.live->stamp[1] = 0u;  // every pair again: the solve's last list does not count
  B.state[pair].active = 1u;  // est, termination and iterations — what write_results_kernel reads — stay as they are
}

__global__ __launch_bounds__(kInfoThreads) void information_kernel(RegBatch B, InfoPartial* __restrict__ partials, uint32_t blocks_per_pair) {
  __shared__ double s_sum[kInfoThreads / 64][kInfoSums];
  __shared__ uint32_t s_cnt[kInfoThreads / 64][4];
  const size_t pair = blockIdx.x / blocks_per_pair;
  const uint32_t blk = blockIdx.x % blocks_per_pair;
  const uint32_t n_se_raw = B.kind[kEdge].n_src[pair * B.in_pitch], n_sp_raw = B.kind[kPlane].n_src[pair * B.in_pitch];
  const uint32_t n_se = n_se_raw < B.kind[kEdge].stride ? n_se_raw : (uint32_t)B.kind[kEdge].stride;
  const uint32_t n_sp = n_sp_raw < B.kind[kPlane].stride ? n_sp_raw : (uint32_t)B.kind[kPlane].stride;
  const uint32_t total = n_se + n_sp;
  const uint32_t base = blk * kInfoChunk;
  if (base >= total) return;  // uniform per workgroup (information_finish_kernel reads the chunks below `total` only)
  const size_t efield = B.n_pairs * B.kind[kEdge].stride, pfield = B.n_pairs * B.kind[kPlane].stride;
  const double* __restrict__ E = B.kind[kEdge].rec + pair * B.kind[kEdge].stride;
  const double* __restrict__ Pl = B.kind[kPlane].rec + pair * B.kind[kPlane].stride;
  InfoAcc acc;
  info_acc_clear(acc);
  // software-pipelined like sweep_kernel: the records of the next two slots are in flight while two are evaluated
  struct Rec {
    double f[9];
    int kind;  // 0 none, 1 edge, 2 plane
  };
  auto load_rec = [&](uint32_t v) {
    Rec R;
    R.kind = 0;
#pragma unroll
    for (int f = 0; f < 9; f++) R.f[f] = 0.0;
    if (v < total) {
      if (v < n_se) {
        R.kind = 1;
#pragma unroll
        for (int f = 0; f < 9; f++) R.f[f] = E[f * efield + v];
      } else {
        const uint32_t q = v - n_se;
        R.kind = 2;
#pragma unroll
        for (int f = 0; f < 7; f++) R.f[f] = Pl[f * pfield + q];
      }
    }
    return R;
  };
  auto eval_rec = [&](const Rec& R) {
    if (R.kind != 0 && R.f[0] == R.f[0]) {  // NaN in field 0 marks an invalid slot
      double prim[6];
#pragma unroll
      for (int f = 0; f < 6; f++) prim[f] = R.f[3 + f];
      info_accumulate(R.kind == 2, v3(R.f[0], R.f[1], R.f[2]), prim, acc);
    }
  };
  Rec c0 = load_rec(base + threadIdx.x), c1 = load_rec(base + kInfoThreads + threadIdx.x);
#pragma unroll 1
  for (int it = 0; it < kInfoItems; it += 2) {
    const bool more = it + 2 < kInfoItems;
    const Rec n0 = more ? load_rec(base + (it + 2) * kInfoThreads + threadIdx.x) : Rec{{0, 0, 0, 0, 0, 0, 0, 0, 0}, 0};
    const Rec n1 = more ? load_rec(base + (it + 3) * kInfoThreads + threadIdx.x) : Rec{{0, 0, 0, 0, 0, 0, 0, 0, 0}, 0};
    eval_rec(c0);
    eval_rec(c1);
    c0 = n0, c1 = n1;
  }
  // wavefront shuffle reduction, then LDS across the 4 wavefronts, fixed order => deterministic
#pragma unroll
  for (int j = 0; j < kInfoSums; j++) {
    double v = acc.s[j];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
    acc.s[j] = v;
  }
  uint32_t cnt[4] = {acc.n_edge, acc.n_plane, acc.n_huber, acc.n_dropped};
#pragma unroll
  for (int j = 0; j < 4; j++) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cnt[j] += __shfl_down(cnt[j], off);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < kInfoSums; j++) s_sum[wave][j] = acc.s[j];
#pragma unroll
    for (int j = 0; j < 4; j++) s_cnt[wave][j] = cnt[j];
  }
  __syncthreads();
  InfoPartial& out = partials[pair * blocks_per_pair + blk];
  if (threadIdx.x < kInfoSums) {
    double v = s_sum[0][threadIdx.x];
    for (int w = 1; w < kInfoThreads / 64; w++) v += s_sum[w][threadIdx.x];
    out.s[threadIdx.x] = v;
  } else if (threadIdx.x < kInfoSums + 4) {
    const int j = threadIdx.x - kInfoSums;
    uint32_t v = s_cnt[0][j];
    for (int w = 1; w < kInfoThreads / 64; w++) v += s_cnt[w][j];
    out.c[j] = v;
  }
}

// one thread per pair: the 6x6 eigen-solve is a few hundred rotations of scalar code (info_eig6)
__global__ __launch_bounds__(64) void information_finish_kernel(RegBatch B, const InfoPartial* __restrict__ partials, uint32_t blocks_per_pair,
                                                                loamx_reg_information* __restrict__ out) {
  const size_t pair = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pair >= B.n_pairs) return;
  const uint32_t n_se_raw = B.kind[kEdge].n_src[pair * B.in_pitch], n_sp_raw = B.kind[kPlane].n_src[pair * B.in_pitch];
  const uint32_t n_se = n_se_raw < B.kind[kEdge].stride ? n_se_raw : (uint32_t)B.kind[kEdge].stride;
  const uint32_t n_sp = n_sp_raw < B.kind[kPlane].stride ? n_sp_raw : (uint32_t)B.kind[kPlane].stride;
  uint32_t used = (n_se + n_sp + kInfoChunk - 1) / kInfoChunk;  // chunks that wrote a partial
  used = used < blocks_per_pair ? used : blocks_per_pair;
  double s[kInfoSums];
  uint32_t c[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < kInfoSums; j++) s[j] = 0.0;
  for (uint32_t b = 0; b < used; b++) {  // chunk order
    const InfoPartial& P = partials[pair * blocks_per_pair + b];
#pragma unroll
    for (int j = 0; j < kInfoSums; j++) s[j] += P.s[j];
#pragma unroll
    for (int j = 0; j < 4; j++) c[j] += P.c[j];
  }
  double H[36], eval[6], evec[36];
  info_mirror(s, H);
  info_eig6(H, eval, evec);
  loamx_reg_information& R = out[pair];
#pragma unroll
  for (int j = 0; j < 36; j++) R.information[j] = H[j], R.eigenvectors[j] = evec[j];
#pragma unroll
  for (int j = 0; j < 6; j++) R.eigenvalues[j] = eval[j], R.gradient[j] = s[21 + j];
  R.weighted_sq_error = s[27];
  R.n_edge = c[0], R.n_plane = c[1], R.n_huber = c[2], R.n_dropped = c[3];
}

}  // namespace

uint32_t info_blocks_per_pair(size_t edge_stride, size_t plane_stride) {
  const size_t b = (edge_stride + plane_stride + kInfoChunk - 1) / kInfoChunk;
  return (uint32_t)(b ? b : 1);
}

void launch_info_activate(const RegBatch& B, hipStream_t s) {
  if (B.n_pairs == 0) return;
  launch_kernel(info_activate_kernel, dim3((unsigned)((B.n_pairs + 63) / 64)), dim3(64), 0, s, B);
}

void launch_information(const RegBatch& B, InfoPartial* partials, loamx_reg_information* d_info, hipStream_t s) {
  if (B.n_pairs == 0) return;
  const uint32_t bpp = info_blocks_per_pair(B.kind[kEdge].stride, B.kind[kPlane].stride);
  launch_kernel(information_kernel, dim3((unsigned)(B.n_pairs * bpp)), dim3(kInfoThreads), 0, s, B, partials, bpp);
  launch_kernel(information_finish_kernel, dim3((unsigned)((B.n_pairs + 63) / 64)), dim3(64), 0, s, B, partials, bpp, d_info);
}

}  // namespace loamx
