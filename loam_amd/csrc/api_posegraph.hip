// api_posegraph.hip — the pose-graph optimiser (loamx.h, "pose graph"): the argument checks, the workspace of a solve, the
// device entry point and the host forms around it.
#include "api_host.h"
#include "posegraph_math.h"

using namespace loamx;

static_assert(sizeof(loamx_pgo_edge) == 352 && sizeof(PgoEdge) == sizeof(loamx_pgo_edge), "loamx_pgo_edge layout");
static_assert(offsetof(loamx_pgo_edge, a_T_b) == offsetof(PgoEdge, z) && offsetof(loamx_pgo_edge, information) == offsetof(PgoEdge, info),
              "loamx_pgo_edge layout");
static_assert(sizeof(loamx_pgo_params) == 48 && sizeof(PgoParams) == sizeof(loamx_pgo_params), "loamx_pgo_params layout");
static_assert(offsetof(loamx_pgo_params, huber_delta) == offsetof(PgoParams, huber_delta), "loamx_pgo_params layout");
static_assert(sizeof(loamx_pgo_summary) == 56 && sizeof(PgoSummary) == sizeof(loamx_pgo_summary), "loamx_pgo_summary layout");
static_assert(offsetof(loamx_pgo_summary, termination) == offsetof(PgoSummary, termination), "loamx_pgo_summary layout");
static_assert(sizeof(loamx_pgo_linearization) == 640 && sizeof(PgoLinearization) == sizeof(loamx_pgo_linearization),
              "loamx_pgo_linearization layout");
static_assert(LOAMX_PGO_COST_CONVERGED == kPgoCostConverged && LOAMX_PGO_STEP_CONVERGED == kPgoStepConverged &&
                  LOAMX_PGO_MAX_ITERATIONS == kPgoMaxIterations && LOAMX_PGO_LAMBDA_OVERFLOW == kPgoLambdaOverflow &&
                  LOAMX_PGO_NOTHING_TO_DO == kPgoNothingToDo && LOAMX_PGO_BAD_INPUT == kPgoBadInput,
              "LOAMX_PGO_* termination codes");

namespace {

constexpr size_t kPgoMaxItems = (size_t)1 << 31;  // poses or edges: an incidence entry is 2 edge + side in 32 bits

int params_check(loamx_ctx* ctx, const loamx_pgo_params* p) {
  if (!p) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null pose-graph parameters");
  const double v[5] = {p->pcg_tolerance, p->initial_lambda, p->cost_tolerance, p->step_tolerance, p->huber_delta};
  for (double x : v)
    if (!isfinite(x)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "a pose-graph parameter is not finite");
  if (p->pcg_tolerance < 0.0 || p->cost_tolerance < 0.0 || p->step_tolerance < 0.0) return fail(ctx, LOAMX_ERR_BAD_PARAM, "a tolerance is negative");
  if (p->huber_delta < 0.0) return fail(ctx, LOAMX_ERR_BAD_PARAM, "huber_delta is negative");
  if (!(p->initial_lambda > 0.0)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "initial_lambda must be positive");
  if (p->max_iterations == 0) return fail(ctx, LOAMX_ERR_BAD_PARAM, "max_iterations must be >= 1");
  return LOAMX_OK;
}

int sizes_check(loamx_ctx* ctx, size_t n_poses, size_t n_edges) {
  if (n_poses >= kPgoMaxItems || n_edges >= kPgoMaxItems) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "2^31 poses or edges or more");
  return LOAMX_OK;
}

// the solve on device arrays (the caller holds ctx->mu, has selected the device and checked the arguments)
int optimize_locked(loamx_ctx* ctx, double* d_poses, size_t n_poses, const uint8_t* d_fixed, const loamx_pgo_edge* d_edges, size_t n_edges,
                    const loamx_pgo_params& params, loamx_pgo_summary* d_summary) {
  untimed(ctx);
  if (n_poses == 0 || n_edges == 0) {
    launch_pgo_nothing(params, d_summary, ctx->stream);
    CHECK_LAUNCH(ctx, "pose-graph summary kernel");
    return LOAMX_OK;
  }
  const PgoLayout L = pgo_layout(n_poses, n_edges);
  ENSURE(ctx, WS_PGO_WORK, L.bytes);
  if (ctx->reg_flags & kRegFlagPoison) HIP_TRY(ctx, hipMemsetAsync(ctx->ws[WS_PGO_WORK].p, 0xFF, L.bytes, ctx->stream));
  launch_pgo_solve(d_poses, n_poses, d_fixed, d_edges, n_edges, params, d_summary, ctx->ws[WS_PGO_WORK].p, ctx->stream);
  CHECK_LAUNCH(ctx, "pose-graph kernels");
  return LOAMX_OK;
}

// what the host forms refuse about the values: non-finite entries and invalid edges
int values_check(loamx_ctx* ctx, const double* poses, size_t n_poses, const loamx_pgo_edge* edges, size_t n_edges) {
  for (size_t i = 0; i < 7 * n_poses; i++)
    if (!isfinite(poses[i])) return fail(ctx, LOAMX_ERR_BAD_PARAM, "a pose is not finite");
  for (size_t e = 0; e < n_edges; e++) {
    if (!pgo_edge_ok(edges[e].a, edges[e].b, n_poses)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "an edge is invalid (a == b, or an end >= n_poses)");
    for (int k = 0; k < 7; k++)
      if (!isfinite(edges[e].a_T_b[k])) return fail(ctx, LOAMX_ERR_BAD_PARAM, "a measurement is not finite");
    for (int i = 0; i < 6; i++)
      for (int j = i; j < 6; j++)
        if (!isfinite(edges[e].information[6 * i + j])) return fail(ctx, LOAMX_ERR_BAD_PARAM, "an information matrix is not finite");
  }
  return LOAMX_OK;
}

}  // namespace

extern "C" {

void loamx_pgo_default_params(loamx_pgo_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->max_iterations = 20, p->max_pcg_iterations = 500, p->pcg_tolerance = 1e-8, p->initial_lambda = 1e-4;
  p->cost_tolerance = 1e-9, p->step_tolerance = 1e-10, p->huber_delta = 0.0;
}

int loamx_pose_graph_optimize_dev(loamx_ctx* ctx, double* d_poses, size_t n_poses, const uint8_t* d_fixed, const loamx_pgo_edge* d_edges,
                                  size_t n_edges, const loamx_pgo_params* params, loamx_pgo_summary* d_summary) {
  API_ENTER(ctx);
  int rc = params_check(ctx, params);
  if (rc == LOAMX_OK) rc = sizes_check(ctx, n_poses, n_edges);
  if (rc != LOAMX_OK) return rc;
  if ((n_poses && !d_poses) || (n_edges && !d_edges)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  return optimize_locked(ctx, d_poses, n_poses, d_fixed, d_edges, n_edges, *params, d_summary);
}

int loamx_pose_graph_optimize(loamx_ctx* ctx, double* poses, size_t n_poses, const uint8_t* fixed, const loamx_pgo_edge* edges, size_t n_edges,
                              const loamx_pgo_params* params, loamx_pgo_summary* summary) {
  API_ENTER(ctx);
  int rc = params_check(ctx, params);
  if (rc == LOAMX_OK) rc = sizes_check(ctx, n_poses, n_edges);
  if (rc != LOAMX_OK) return rc;
  if (!summary || (n_poses && !poses) || (n_edges && !edges)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  rc = values_check(ctx, poses, n_poses, edges, n_edges);
  if (rc != LOAMX_OK) return rc;
  if (fixed && n_poses) {
    bool any = false;
    for (size_t i = 0; i < n_poses && !any; i++) any = fixed[i] != 0;
    if (!any) return fail(ctx, LOAMX_ERR_BAD_PARAM, "no pose is fixed");
  }
  untimed(ctx);
  ENSURE(ctx, WS_PGO_OUT, sizeof(loamx_pgo_summary));
  const bool solve = n_poses && n_edges;
  if (solve) {
    ENSURE(ctx, WS_PGO_POSES, n_poses * 7 * sizeof(double));
    ENSURE(ctx, WS_PGO_EDGES, n_edges * sizeof(loamx_pgo_edge));
    if (fixed) ENSURE(ctx, WS_PGO_FIXED, n_poses);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[WS_PGO_POSES].p, poses, n_poses * 7 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[WS_PGO_EDGES].p, edges, n_edges * sizeof(loamx_pgo_edge), hipMemcpyHostToDevice, ctx->stream));
    if (fixed) HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[WS_PGO_FIXED].p, fixed, n_poses, hipMemcpyHostToDevice, ctx->stream));
  }
  rc = optimize_locked(ctx, solve ? wsp<double>(ctx, WS_PGO_POSES) : nullptr, solve ? n_poses : 0, solve && fixed ? wsp<uint8_t>(ctx, WS_PGO_FIXED) : nullptr,
                       solve ? wsp<loamx_pgo_edge>(ctx, WS_PGO_EDGES) : nullptr, solve ? n_edges : 0, *params, wsp<loamx_pgo_summary>(ctx, WS_PGO_OUT));
  if (rc != LOAMX_OK) {
    (void)hipStreamSynchronize(ctx->stream);  // (the uploads must not outlive the caller's arrays)
    return rc;
  }
  loamx_pgo_summary got;
  HIP_TRY(ctx, hipMemcpyAsync(&got, ctx->ws[WS_PGO_OUT].p, sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  // (a solve that accepted nothing left the device copy as it was uploaded: the read-back then returns the caller's own bytes)
  if (solve) HIP_TRY(ctx, hipMemcpy(poses, ctx->ws[WS_PGO_POSES].p, n_poses * 7 * sizeof(double), hipMemcpyDeviceToHost));
  *summary = got;
  return LOAMX_OK;
}

int loamx_pose_graph_linearize(loamx_ctx* ctx, const double* poses, size_t n_poses, const loamx_pgo_edge* edges, size_t n_edges,
                               double huber_delta, loamx_pgo_linearization* out) {
  API_ENTER(ctx);
  int rc = sizes_check(ctx, n_poses, n_edges);
  if (rc != LOAMX_OK) return rc;
  if (!isfinite(huber_delta) || huber_delta < 0.0) return fail(ctx, LOAMX_ERR_BAD_PARAM, "huber_delta must be finite and not negative");
  if (n_edges == 0) return LOAMX_OK;
  if (!poses || !edges || !out) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  rc = values_check(ctx, poses, n_poses, edges, n_edges);
  if (rc != LOAMX_OK) return rc;
  untimed(ctx);
  ENSURE(ctx, WS_PGO_POSES, n_poses * 7 * sizeof(double));
  ENSURE(ctx, WS_PGO_EDGES, n_edges * sizeof(loamx_pgo_edge));
  ENSURE(ctx, WS_PGO_OUT, n_edges * sizeof(loamx_pgo_linearization));
  ENSURE(ctx, WS_PGO_WORK, pgo_readout_ws_bytes(n_edges));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[WS_PGO_POSES].p, poses, n_poses * 7 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[WS_PGO_EDGES].p, edges, n_edges * sizeof(loamx_pgo_edge), hipMemcpyHostToDevice, ctx->stream));
  launch_pgo_linearize_readout(wsp<double>(ctx, WS_PGO_POSES), wsp<loamx_pgo_edge>(ctx, WS_PGO_EDGES), n_edges, huber_delta,
                               wsp<loamx_pgo_linearization>(ctx, WS_PGO_OUT), wsp<double>(ctx, WS_PGO_WORK), ctx->stream);
  rc = check_launch(ctx, "pose-graph linearisation kernel");
  if (rc != LOAMX_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  HIP_TRY(ctx, hipMemcpyAsync(out, ctx->ws[WS_PGO_OUT].p, n_edges * sizeof(loamx_pgo_linearization), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LOAMX_OK;
}

int loamx_pose_graph_edges_from_results_dev(loamx_ctx* ctx, const loamx_reg_result* d_results, const loamx_reg_information* d_info,
                                            size_t n_pairs, uint32_t first_id, loamx_pgo_edge* d_edges) {
  API_ENTER(ctx);
  if (n_pairs == 0) return LOAMX_OK;
  if (!d_results || !d_info || !d_edges) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  if (n_pairs >= kPgoMaxItems || (size_t)first_id + n_pairs >= kPgoMaxItems) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "pose ids beyond 2^31");
  untimed(ctx);
  launch_pgo_edges_from_results(d_results, d_info, n_pairs, first_id, d_edges, ctx->stream);
  CHECK_LAUNCH(ctx, "pose-graph edge kernel");
  return LOAMX_OK;
}

}  // extern "C"
