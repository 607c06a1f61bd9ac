// api_sequence.hip — scans in, poses out: extraction and registration of scan pairs and scan sequences in one call (device
// resident, or streamed from host memory in chunks), the trajectory of the results, motion correction of scans.
#include "api_host.h"

using namespace loamx;

extern "C" {

// How the scans of a call lie in memory. Interleaved pairs: n_pairs x 2 scans, pair p = (scan 2p target, scan 2p + 1 source).
// Sequence: n_pairs + 1 scans, pair p = (scan p target, scan p + 1 source) — every scan is extracted ONCE and read in both roles.
enum class ScanLayout { kPairs, kSequence };
// (the caller holds ctx->mu and has selected the device; `look` = refuse non-finite input whatever CHECK_FINITE says;
// d_init: n_pairs x 7 doubles or nullptr = identity)
static int register_scan_pairs_locked(loamx_ctx* ctx, const void* d_xyz, bool f32, size_t n_pairs, const loamx_lidar_params* lidar,
                                      const loamx_fe_params* fe, const loamx_reg_params* reg, loamx_reg_result* d_results, bool look,
                                      ScanLayout layout, const double* d_init, loamx_reg_information* d_info) {
  ExtractParams P;
  int rc = make_extract_params(ctx, lidar, fe, P);
  if (rc != LOAMX_OK) return rc;
  RegConfig C;
  rc = make_reg_config(ctx, reg, C);
  if (rc != LOAMX_OK) return rc;
  if (n_pairs == 0) return LOAMX_OK;
  const bool seq = layout == ScanLayout::kSequence;
  const size_t n_scans = seq ? n_pairs + 1 : 2 * n_pairs, ecap = edge_capacity(P), pcap = planar_capacity(P);
  rc = dev_check_finite(ctx, d_xyz, f32, nullptr, n_scans, (size_t)P.H * P.W, 1, look);
  if (rc != LOAMX_OK) return rc;
  if (d_init && (look || (ctx->reg_flags & kRegFlagCheckFinite))) {
    rc = check_finite_scalars(ctx, d_init, n_pairs * 7);
    if (rc != LOAMX_OK) return rc;
  }
  const size_t cap[2] = {ecap, pcap};
  for (int k = 0; k < 2; k++) ENSURE(ctx, ctx->wsk[WSK_N][k], n_scans * sizeof(uint32_t));
  for (int k = 0; k < 2; k++) ENSURE(ctx, ctx->wsk[WSK_XYZ][k], n_scans * cap[k] * 3 * sizeof(double));
  ExtractBoxes boxes;
  // (no index arrays: the registration reads the features' points, and 4 bytes per feature are 0.15 GB per 1 024-pair step)
  rc = extract_dev(ctx, d_xyz, f32, n_scans, P, nullptr, wskp<uint32_t>(ctx, WSK_N, kEdge), wskp<double>(ctx, WSK_XYZ, kEdge), nullptr,
                   wskp<uint32_t>(ctx, WSK_N, kPlane), wskp<double>(ctx, WSK_XYZ, kPlane), false, &boxes);
  if (rc != LOAMX_OK) return rc;
  // interleaved: scan 2p = target, scan 2p + 1 = source (in_pitch 2); sequence: scan p = target, scan p + 1 = source (in_pitch 1).
  // Either way a pair's source lies ONE scan behind its target: features, counts and boxes alike.
  RegInputs in{};
  in.boxes = boxes, in.src_box_offset = 1;
  in.n_pairs = n_pairs, in.in_pitch = seq ? 1 : 2;
  for (int k = 0; k < 2; k++) {
    const double* xyz = wskp<double>(ctx, WSK_XYZ, k);
    const uint32_t* count = wskp<uint32_t>(ctx, WSK_N, k);
    in.kind[k] = RegInputs::Kind{cap[k], xyz + cap[k] * 3, xyz, count + 1, count};
  }
  in.init = d_init;
  // the registration; with d_info, the information matrices at its final estimates behind it
  RegPrepareOpts opts{};
  opts.want_info_partials = d_info != nullptr;
  RegBatch B;
  rc = reg_prepare(ctx, in, C, nullptr, opts, B);
  if (rc != LOAMX_OK) return rc;
  rc = reg_solve(ctx, B, C, d_results, nullptr, nullptr);
  if (rc != LOAMX_OK || !d_info) return rc;
  return reg_information(ctx, B, C, reg_info_partials(ctx), d_info, true);
}
static int register_scan_pairs(loamx_ctx* ctx, const void* d_xyz, bool f32, size_t n_pairs, const loamx_lidar_params* lidar,
                               const loamx_fe_params* fe, const loamx_reg_params* reg, loamx_reg_result* d_results,
                               ScanLayout layout, const double* d_init, loamx_reg_information* d_info) {
  API_ENTER(ctx);
  return register_scan_pairs_locked(ctx, d_xyz, f32, n_pairs, lidar, fe, reg, d_results, false, layout, d_init, d_info);
}

// Host memory in, host memory out (loamx.h: loamx_register_scan_pairs): chunk k + 1 is uploaded on the copy stream into the
// other staging buffer while chunk k goes through register_scan_pairs_locked — the host blocks inside that call (its two
// read-backs), so the next upload is enqueued BEFORE it; a buffer is refilled once the chunk that read it has finished.
// Sequence layout (loamx_register_scan_sequence): chunk k of C pairs uploads the C + 1 scans k C .. k C + C it reads; the scan two
// neighbouring chunks share travels and is extracted twice (1 / C extra), so the chunks stay independent of each other.
// init: n_pairs x 7 host doubles or nullptr; uploaded once, in front of the first chunk.
constexpr size_t kStreamChunkPairs = 128;
static int register_scan_pairs_host(loamx_ctx* ctx, const void* xyz, bool f32, size_t n_pairs, const loamx_lidar_params* lidar,
                                    const loamx_fe_params* fe, const loamx_reg_params* reg, loamx_reg_result* results,
                                    ScanLayout layout = ScanLayout::kPairs, const double* init = nullptr) {
  API_ENTER(ctx);
  {  // (parameter errors before anything moves)
    ExtractParams P;
    int rc = make_extract_params(ctx, lidar, fe, P);
    if (rc != LOAMX_OK) return rc;
    RegConfig C;
    rc = make_reg_config(ctx, reg, C);
    if (rc != LOAMX_OK) return rc;
  }
  if (n_pairs == 0) return LOAMX_OK;
  if (!xyz || !results) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  const bool seq = layout == ScanLayout::kSequence;
  const size_t scan_bytes = (size_t)lidar->scan_lines * lidar->points_per_line * 3 * (f32 ? sizeof(float) : sizeof(double));
  const size_t pair_bytes = (seq ? 1 : 2) * scan_bytes;  // from one pair's target scan to the next pair's
  const size_t tail_bytes = seq ? scan_bytes : 0;        // the source scan of a chunk's last pair (sequence)
  size_t chunk = ctx->stream_chunk_pairs > 0 ? (size_t)ctx->stream_chunk_pairs : kStreamChunkPairs;
  chunk = chunk < n_pairs ? chunk : n_pairs;
  const size_t n_chunks = (n_pairs + chunk - 1) / chunk;
  untimed(ctx);
  ENSURE(ctx, WS_STREAM_IN0, chunk * pair_bytes + tail_bytes);
  if (n_chunks > 1) ENSURE(ctx, WS_STREAM_IN1, chunk * pair_bytes + tail_bytes);
  ENSURE(ctx, WS_STREAM_RES, n_pairs * sizeof(loamx_reg_result));
  if (init) ENSURE(ctx, WS_STREAM_INIT, n_pairs * 7 * sizeof(double));
  // (each handle on its own: a creation that failed half-way in an earlier call must not leave the others null for good)
  if (!ctx->copy_stream) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
  for (int b = 0; b < 2; b++) {
    if (!ctx->ev_up[b]) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_up[b], hipEventDisableTiming));
    if (!ctx->ev_free[b]) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_free[b], hipEventDisableTiming));
  }
  unsigned char* in[2] = {wsp<unsigned char>(ctx, WS_STREAM_IN0), n_chunks > 1 ? wsp<unsigned char>(ctx, WS_STREAM_IN1) : nullptr};
  loamx_reg_result* d_res = wsp<loamx_reg_result>(ctx, WS_STREAM_RES);
  const unsigned char* host = static_cast<const unsigned char*>(xyz);
  auto pairs_of = [&](size_t k) { return k + 1 < n_chunks ? chunk : n_pairs - k * chunk; };
  auto upload = [&](size_t k) -> hipError_t {
    const int b = (int)(k & 1);
    hipError_t e = hipSuccess;
    if (k >= 2) e = hipStreamWaitEvent(ctx->copy_stream, ctx->ev_free[b], 0);  // (the chunk that read this buffer is done)
    if (e == hipSuccess) e = hipMemcpyAsync(in[b], host + k * chunk * pair_bytes, pairs_of(k) * pair_bytes + tail_bytes, hipMemcpyHostToDevice, ctx->copy_stream);
    if (e == hipSuccess) e = hipEventRecord(ctx->ev_up[b], ctx->copy_stream);
    return e;
  };
  // (whatever earlier calls left on the context's stream may still read the staging buffers' neighbours: nothing to wait for,
  // the buffers are this entry point's own — but a previous call of THIS entry point has synchronised before it returned)
  // (whatever fails below: uploads in flight must not outlive the caller's buffer, nor the staging buffers a later call may grow)
  auto drain = [&](int code) {
    (void)hipStreamSynchronize(ctx->copy_stream);
    (void)hipStreamSynchronize(ctx->stream);
    return code;
  };
#define STREAM_TRY(expr)                                                                                  \
  do {                                                                                                    \
    hipError_t e_ = (expr);                                                                               \
    if (e_ != hipSuccess) return drain(fail(ctx, LOAMX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_))); \
  } while (0)
  STREAM_TRY(upload(0));
  double* d_init = init ? wsp<double>(ctx, WS_STREAM_INIT) : nullptr;
  if (init) STREAM_TRY(hipMemcpyAsync(d_init, init, n_pairs * 7 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  int rc = LOAMX_OK;
  for (size_t k = 0; k < n_chunks && rc == LOAMX_OK; k++) {
    const int b = (int)(k & 1);
    if (k + 1 < n_chunks) STREAM_TRY(upload(k + 1));
    STREAM_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_up[b], 0));
    rc = register_scan_pairs_locked(ctx, in[b], f32, pairs_of(k), lidar, fe, reg, d_res + k * chunk, true, layout, d_init ? d_init + k * chunk * 7 : nullptr, nullptr);
    untimed(ctx);
    if (rc == LOAMX_OK) STREAM_TRY(hipEventRecord(ctx->ev_free[b], ctx->stream));
  }
  if (rc != LOAMX_OK) return drain(rc);
  STREAM_TRY(hipMemcpyAsync(results, d_res, n_pairs * sizeof(loamx_reg_result), hipMemcpyDeviceToHost, ctx->stream));
  STREAM_TRY(hipStreamSynchronize(ctx->stream));
  return LOAMX_OK;
#undef STREAM_TRY
}

int loamx_register_scan_pairs(loamx_ctx* ctx, const double* xyz, size_t n_pairs, const loamx_lidar_params* lidar,
                              const loamx_fe_params* fe, const loamx_reg_params* reg, loamx_reg_result* results) {
  return register_scan_pairs_host(ctx, xyz, false, n_pairs, lidar, fe, reg, results);
}
int loamx_register_scan_pairs_f32(loamx_ctx* ctx, const float* xyz, size_t n_pairs, const loamx_lidar_params* lidar,
                                  const loamx_fe_params* fe, const loamx_reg_params* reg, loamx_reg_result* results) {
  return register_scan_pairs_host(ctx, xyz, true, n_pairs, lidar, fe, reg, results);
}

int loamx_register_scan_pairs_dev(loamx_ctx* ctx, const double* d_xyz, size_t n_pairs, const loamx_lidar_params* lidar,
                                  const loamx_fe_params* fe, const loamx_reg_params* reg, loamx_reg_result* d_results) {
  return register_scan_pairs(ctx, d_xyz, false, n_pairs, lidar, fe, reg, d_results, ScanLayout::kPairs, nullptr, nullptr);
}

int loamx_register_scan_pairs_dev_f32(loamx_ctx* ctx, const float* d_xyz, size_t n_pairs, const loamx_lidar_params* lidar,
                                      const loamx_fe_params* fe, const loamx_reg_params* reg, loamx_reg_result* d_results) {
  return register_scan_pairs(ctx, d_xyz, true, n_pairs, lidar, fe, reg, d_results, ScanLayout::kPairs, nullptr, nullptr);
}

// (the "_info" forms: the same static helpers with a place for the information records)
static int register_scan_pairs_info(loamx_ctx* ctx, const void* d_xyz, bool f32, size_t n_pairs, const loamx_lidar_params* lidar,
                                    const loamx_fe_params* fe, const loamx_reg_params* reg, loamx_reg_result* d_results, ScanLayout layout,
                                    const double* d_init, loamx_reg_information* d_info) {
  if (!ctx) return LOAMX_ERR_BAD_PARAM;
  if (n_pairs != 0 && (!d_info || !d_results || !d_xyz)) {
    ApiLock lock(ctx);
    return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  }
  return register_scan_pairs(ctx, d_xyz, f32, n_pairs, lidar, fe, reg, d_results, layout, d_init, d_info);
}
int loamx_register_scan_pairs_info_dev(loamx_ctx* ctx, const double* d_xyz, size_t n_pairs, const loamx_lidar_params* lidar,
                                       const loamx_fe_params* fe, const loamx_reg_params* reg, loamx_reg_result* d_results,
                                       loamx_reg_information* d_info) {
  return register_scan_pairs_info(ctx, d_xyz, false, n_pairs, lidar, fe, reg, d_results, ScanLayout::kPairs, nullptr, d_info);
}
int loamx_register_scan_pairs_info_dev_f32(loamx_ctx* ctx, const float* d_xyz, size_t n_pairs, const loamx_lidar_params* lidar,
                                           const loamx_fe_params* fe, const loamx_reg_params* reg, loamx_reg_result* d_results,
                                           loamx_reg_information* d_info) {
  return register_scan_pairs_info(ctx, d_xyz, true, n_pairs, lidar, fe, reg, d_results, ScanLayout::kPairs, nullptr, d_info);
}
int loamx_register_scan_sequence_info_dev(loamx_ctx* ctx, const double* d_xyz, size_t n_scans, const loamx_lidar_params* lidar,
                                          const loamx_fe_params* fe, const loamx_reg_params* reg, const double* d_init,
                                          loamx_reg_result* d_results, loamx_reg_information* d_info) {
  return register_scan_pairs_info(ctx, d_xyz, false, n_scans < 2 ? 0 : n_scans - 1, lidar, fe, reg, d_results, ScanLayout::kSequence, d_init, d_info);
}
int loamx_register_scan_sequence_info_dev_f32(loamx_ctx* ctx, const float* d_xyz, size_t n_scans, const loamx_lidar_params* lidar,
                                              const loamx_fe_params* fe, const loamx_reg_params* reg, const double* d_init,
                                              loamx_reg_result* d_results, loamx_reg_information* d_info) {
  return register_scan_pairs_info(ctx, d_xyz, true, n_scans < 2 ? 0 : n_scans - 1, lidar, fe, reg, d_results, ScanLayout::kSequence, d_init, d_info);
}

/* ---- scan sequences: scan i is the source of pair i - 1 and the target of pair i ----------------------------- */
int loamx_register_scan_sequence_dev(loamx_ctx* ctx, const double* d_xyz, size_t n_scans, const loamx_lidar_params* lidar,
                                     const loamx_fe_params* fe, const loamx_reg_params* reg, const double* d_init, loamx_reg_result* d_results) {
  return register_scan_pairs(ctx, d_xyz, false, n_scans < 2 ? 0 : n_scans - 1, lidar, fe, reg, d_results, ScanLayout::kSequence, d_init, nullptr);
}
int loamx_register_scan_sequence_dev_f32(loamx_ctx* ctx, const float* d_xyz, size_t n_scans, const loamx_lidar_params* lidar,
                                         const loamx_fe_params* fe, const loamx_reg_params* reg, const double* d_init, loamx_reg_result* d_results) {
  return register_scan_pairs(ctx, d_xyz, true, n_scans < 2 ? 0 : n_scans - 1, lidar, fe, reg, d_results, ScanLayout::kSequence, d_init, nullptr);
}
int loamx_register_scan_sequence(loamx_ctx* ctx, const double* xyz, size_t n_scans, const loamx_lidar_params* lidar, const loamx_fe_params* fe,
                                 const loamx_reg_params* reg, const double* init, loamx_reg_result* results) {
  return register_scan_pairs_host(ctx, xyz, false, n_scans < 2 ? 0 : n_scans - 1, lidar, fe, reg, results, ScanLayout::kSequence, init);
}
int loamx_register_scan_sequence_f32(loamx_ctx* ctx, const float* xyz, size_t n_scans, const loamx_lidar_params* lidar, const loamx_fe_params* fe,
                                     const loamx_reg_params* reg, const double* init, loamx_reg_result* results) {
  return register_scan_pairs_host(ctx, xyz, true, n_scans < 2 ? 0 : n_scans - 1, lidar, fe, reg, results, ScanLayout::kSequence, init);
}

int loamx_compose_trajectory_dev(loamx_ctx* ctx, const loamx_reg_result* d_results, size_t n_pairs, const double origin[7], double* d_world_T_scan) {
  API_ENTER(ctx);
  if (!d_world_T_scan || (n_pairs && !d_results)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  const double identity[7] = {0, 0, 0, 1, 0, 0, 0};
  if (origin && !host_all_finite(origin, false, 7)) return fail(ctx, LOAMX_ERR_BAD_PARAM, kNonFiniteMsg);
  untimed(ctx);
  launch_trajectory(d_results, n_pairs, origin ? origin : identity, d_world_T_scan, ctx->stream);
  CHECK_LAUNCH(ctx, "trajectory_kernel");
  return LOAMX_OK;
}

static int deskew_scans_dev(loamx_ctx* ctx, const void* d_xyz, bool f32, size_t n_scans, const loamx_lidar_params* lidar, const double* d_motion,
                            double ref_fraction, void* d_xyz_out) {
  API_ENTER(ctx);
  if (!lidar) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null parameter struct");
  if (!(ref_fraction >= 0.0 && ref_fraction <= 1.0)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "ref_fraction must lie in [0, 1]");
  if (lidar->scan_lines > 0xFFFFFFFFull || lidar->points_per_line > 0xFFFFFFFFull)
    return fail(ctx, LOAMX_ERR_UNSUPPORTED, "scan too large for 32-bit line and column numbers");
  if (n_scans == 0 || lidar->scan_lines == 0 || lidar->points_per_line == 0) return LOAMX_OK;
  if (!d_xyz || !d_motion || !d_xyz_out) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  if (n_scans * ((lidar->points_per_line + 255) / 256) > 0x7FFFFFFFull) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "too many scans in one call");
  if (ctx->reg_flags & kRegFlagCheckFinite) {  // (the motions; non-finite POINTS are defined here: copied unchanged)
    int rc = check_finite_scalars(ctx, d_motion, n_scans * 7);
    if (rc != LOAMX_OK) return rc;
  }
  untimed(ctx);
  launch_deskew(d_xyz, d_xyz_out, f32, n_scans, (uint32_t)lidar->scan_lines, (uint32_t)lidar->points_per_line, d_motion, ref_fraction, ctx->stream);
  CHECK_LAUNCH(ctx, "deskew_kernel");
  return LOAMX_OK;
}
int loamx_deskew_scans_dev(loamx_ctx* ctx, const double* d_xyz, size_t n_scans, const loamx_lidar_params* lidar, const double* d_motion,
                           double ref_fraction, double* d_xyz_out) {
  return deskew_scans_dev(ctx, d_xyz, false, n_scans, lidar, d_motion, ref_fraction, d_xyz_out);
}
int loamx_deskew_scans_dev_f32(loamx_ctx* ctx, const float* d_xyz, size_t n_scans, const loamx_lidar_params* lidar, const double* d_motion,
                               double ref_fraction, float* d_xyz_out) {
  return deskew_scans_dev(ctx, d_xyz, true, n_scans, lidar, d_motion, ref_fraction, d_xyz_out);
}
int loamx_deskew_launch_geometry(size_t n_scans, uint64_t scan_lines, uint64_t points_per_line, uint32_t out[4]) {
  if (!out) return LOAMX_ERR_BAD_PARAM;
  if (scan_lines > 0xFFFFFFFFull || points_per_line > 0xFFFFFFFFull || n_scans * ((points_per_line + 255) / 256) > 0x7FFFFFFFull)
    return LOAMX_ERR_UNSUPPORTED;  // (what deskew_scans_dev refuses)
  const DeskewGeometry g = deskew_launch_geometry(n_scans, (uint32_t)scan_lines, (uint32_t)points_per_line);
  out[0] = g.col_blocks, out[1] = g.groups, out[2] = g.lines_per_block, out[3] = g.unroll;
  return LOAMX_OK;
}

}  // extern "C"
