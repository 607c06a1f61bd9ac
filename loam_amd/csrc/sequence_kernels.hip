// sequence_kernels.hip — what a scan SEQUENCE needs beyond the pair pipeline (loamx.h: loamx_compose_trajectory_dev,
// loamx_deskew_scans_dev): the chained trajectory of the per-pair results and the per-point motion correction of a batch
// of scans (deskew_math.h).
#include "loamx_internal.h"
#include "deskew_math.h"

namespace loamx {
namespace {

/* ---- de-skew -------------------------------------------------------------------------------------------------------
 * A stream: every point is read once and written once (24 + 24 B, 12 + 12 B for float scans). One thread per column:
 * its rotation and offset (two sincos pairs, one 3 x 3 product) depend on (scan, column) only, so the thread computes
 * them once and walks down the scan lines of its workgroup's share with them. Consecutive lanes hold consecutive
 * columns: the three loads of a wavefront cover 64 adjacent points (1 536 contiguous bytes) between them, the stores
 * likewise. blockIdx.x = scan * column blocks + column block, blockIdx.y = share of the lines (the launcher splits the
 * lines until the grid has enough workgroups for the chip, see launch_deskew). In place (out == in) is fine: a thread
 * reads a point before it writes that point and nobody else touches it — hence no __restrict__ on the two arrays. */
constexpr int kDeskewThreads = 256;
constexpr int kDeskewUnroll = 4;  // lines in flight per thread

template <typename T>
__global__ __launch_bounds__(kDeskewThreads) void deskew_kernel(const T* xyz, T* out, const double* __restrict__ motion, uint32_t H, uint32_t W,
                                                                 uint32_t col_blocks, uint32_t lines_per_block, double rho) {
  const uint32_t scan = blockIdx.x / col_blocks, cb = blockIdx.x - scan * col_blocks;
  const uint32_t col = cb * kDeskewThreads + threadIdx.x;
  if (col >= W) return;
  const uint32_t l0 = blockIdx.y * lines_per_block;
  const uint32_t l1 = l0 + lines_per_block < H ? l0 + lines_per_block : H;
  double q[4], t[3];
  deskew_load_motion(motion + (size_t)scan * 7, q, t);
  const DeskewColumn c = deskew_column(q, t, (double)col / (double)W, rho);
  const size_t base = ((size_t)scan * H * W + col) * 3, pitch = (size_t)W * 3;
  for (uint32_t l = l0; l < l1; l += kDeskewUnroll) {
    T v[kDeskewUnroll][3];
#pragma unroll
    for (int u = 0; u < kDeskewUnroll; u++) {
      if (l + u < l1) {
        const T* p = xyz + base + (size_t)(l + u) * pitch;
        v[u][0] = p[0], v[u][1] = p[1], v[u][2] = p[2];
      }
    }
#pragma unroll
    for (int u = 0; u < kDeskewUnroll; u++) {
      if (l + u < l1) {
        double r[3];
        T* o = out + base + (size_t)(l + u) * pitch;
        if (deskew_point(c, (double)v[u][0], (double)v[u][1], (double)v[u][2], r)) o[0] = (T)r[0], o[1] = (T)r[1], o[2] = (T)r[2];
        else o[0] = v[u][0], o[1] = v[u][1], o[2] = v[u][2];
      }
    }
  }
}

/* ---- trajectory ----------------------------------------------------------------------------------------------------
 * world_T_scan[0] = origin, world_T_scan[i + 1] = world_T_scan[i] (+) results[i].pose (reg_math.h: pose_compose, the
 * arithmetic of Pose3d::compose). One wavefront: the lanes fetch 64 records and store 64 poses at a time, lane 0 walks
 * the chain in between — the reference loop's own order, so the bits are those of that loop and the same on every run.
 * The chain is the whole cost (about a hundred dependent FP64 operations per pose); 4 096 poses take well under a
 * millisecond, next to the registrations that produced them. */
struct Pose7 {
  double v[7];
};
__global__ __launch_bounds__(64) void trajectory_kernel(const loamx_reg_result* __restrict__ results, size_t n_pairs, Pose7 origin,
                                                        double* __restrict__ world_T_scan) {
  __shared__ double s_in[64][7], s_out[64][7];
  const uint32_t lane = threadIdx.x;
  double cur[7];
  for (int k = 0; k < 7; k++) cur[k] = origin.v[k];
  if (lane == 0)
    for (int k = 0; k < 7; k++) world_T_scan[k] = cur[k];
  for (size_t b = 0; b < n_pairs; b += 64) {
    const uint32_t n = n_pairs - b < 64 ? (uint32_t)(n_pairs - b) : 64u;
    if (lane < n)
      for (int k = 0; k < 7; k++) s_in[lane][k] = results[b + lane].pose[k];
    __syncthreads();
    if (lane == 0) {
      for (uint32_t i = 0; i < n; i++) {
        double step[7], next[7];
        for (int k = 0; k < 7; k++) step[k] = s_in[i][k];
        pose_compose(cur, step, next);
        for (int k = 0; k < 7; k++) cur[k] = next[k], s_out[i][k] = next[k];
      }
    }
    __syncthreads();
    if (lane < n)
      for (int k = 0; k < 7; k++) world_T_scan[(b + 1 + lane) * 7 + k] = s_out[lane][k];
  }
}

}  // namespace

// The shape of the de-skew launch (loamx_deskew_launch_geometry): the one place that decides it.
// enough workgroups for 256 compute units several times over, also for a single scan: the lines are split as far as
// that takes (a thread that walks fewer lines amortises its column's sincos over fewer points)
DeskewGeometry deskew_launch_geometry(size_t n_scans, uint32_t H, uint32_t W) {
  DeskewGeometry g{0, 0, 0, (uint32_t)kDeskewUnroll};
  if (n_scans == 0 || H == 0 || W == 0) return g;
  g.col_blocks = (W + kDeskewThreads - 1) / kDeskewThreads;
  const size_t wide = (size_t)g.col_blocks * n_scans;
  uint32_t groups = (uint32_t)((2048 + wide - 1) / wide);
  groups = groups < 1u ? 1u : (groups > H ? H : groups);
  g.lines_per_block = (H + groups - 1) / groups;
  g.groups = (H + g.lines_per_block - 1) / g.lines_per_block;
  return g;
}

// d_xyz / d_out: n_scans x H x W x 3 scalars (float when f32); the caller has checked that the grid fits
void launch_deskew(const void* d_xyz, void* d_out, bool f32, size_t n_scans, uint32_t H, uint32_t W, const double* d_motion, double rho,
                   hipStream_t s) {
  if (n_scans == 0 || H == 0 || W == 0) return;
  const DeskewGeometry g = deskew_launch_geometry(n_scans, H, W);
  const uint32_t col_blocks = g.col_blocks, groups = g.groups, lines_per_block = g.lines_per_block;
  const size_t wide = (size_t)col_blocks * n_scans;
  const dim3 grid((unsigned)wide, groups);
  if (f32)
    launch_kernel(deskew_kernel<float>, grid, dim3(kDeskewThreads), 0, s, static_cast<const float*>(d_xyz), static_cast<float*>(d_out), d_motion, H, W,
                  col_blocks, lines_per_block, rho);
  else
    launch_kernel(deskew_kernel<double>, grid, dim3(kDeskewThreads), 0, s, static_cast<const double*>(d_xyz), static_cast<double*>(d_out), d_motion, H,
                  W, col_blocks, lines_per_block, rho);
}

void launch_trajectory(const loamx_reg_result* d_results, size_t n_pairs, const double origin[7], double* d_world_T_scan, hipStream_t s) {
  Pose7 o;
  for (int k = 0; k < 7; k++) o.v[k] = origin[k];
  launch_kernel(trajectory_kernel, dim3(1), dim3(64), 0, s, d_results, n_pairs, o, d_world_T_scan);
}

}  // namespace loamx
