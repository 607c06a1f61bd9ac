// localize_math.h — scan-to-map localisation on a surfel map (loamx.h, "surfel localisation"): the candidate voxels of a moved
// point, the usable test, the choice, the gate, the Huber-scaled point-to-plane row, the 28 ordered sums, and the solve of one
// iteration (eigen-remapped Gauss-Newton step, left retraction, the decisions). Host + device: the kernels of
// localize_kernels.hip and the host loop of tests/hostcheck_localize call the same functions. Every product, quotient, sum and
// difference is rounded on its own (-ffp-contract=off), in the order written; sqrt is the only libm call. What surfel_math.h
// (surfel_finish, surfel_distance) and info_math.h (InfoRow, info_mirror, info_eig6) have is used from there, not restated.
//
// THE ROW. The subtraction happens first: s = surfel_distance(plane, v) = normal . (v - mean) — the gate's own s — then r = |s|,
// g = copysign(1, s) normal, J = [v x g, g]. (info_row's plane form, s = n . v - d, would round differently from the gate.)
#pragma once
#include "info_math.h"
#include "surfel_math.h"

namespace loamx {

constexpr int kLocThreads = 256;                          // threads of an accumulate workgroup
constexpr int kLocItems = 16;                             // points per thread of a chunk
constexpr uint32_t kLocChunk = kLocThreads * kLocItems;   // points per chunk of a cloud: one partial each
constexpr int kLocCandidates = 7;                         // the home voxel, then -x +x -y +y -z +z
constexpr uint32_t kLocMaxIterations = 1000;
// loamx.h: LOAMX_LOCALIZE_* (api_localize.hip asserts the equality)
constexpr uint32_t kLocConverged = 0, kLocMaxIter = 1, kLocTooFewRows = 2, kLocNotFinite = 3;
// the counters of an evaluation, in the order of LocAcc::c
enum { kLocRows = 0, kLocHuber = 1, kLocNoSurfel = 2, kLocGated = 3, kLocUnused = 4, kLocCounters = 5 };

// what a candidate voxel offers a point: 64 bytes, the record of the localiser's plane cache
struct alignas(64) LocPlane {
  double mean[3];
  double normal[3];
  uint32_t count, usable;
  uint32_t pad[2];
};

// the rule of a call (api_localize.hip fills it from loamx_localize_params and the map's own leaf and ranges)
struct LocRule {
  double leaf, min_r2, max_r2;
  double planarity, max_distance, huber_delta;
  uint32_t min_points, neighborhood;
};
// the solve's share of the parameters
struct LocSolve {
  double rot_thresh, pos_thresh, min_eig_per_row;
  uint32_t max_iterations, min_rows;
};

// THE usable test of a voxel that has a slot (no division)
LOAMX_HD bool loc_usable(uint32_t count, double eval0, double eval1, uint32_t min_points, double planarity) {
  return count != 0u && count >= min_points && eval1 > 0.0 && eval0 <= planarity * eval1;
}
LOAMX_HD LocPlane loc_plane_of(const loamx_surfel& r, uint32_t min_points, double planarity) {
  LocPlane p;
#pragma unroll
  for (int a = 0; a < 3; a++) p.mean[a] = r.mean[a], p.normal[a] = r.normal[a];
  p.count = r.count, p.usable = loc_usable(r.count, r.eval[0], r.eval[1], min_points, planarity) ? 1u : 0u;
  p.pad[0] = p.pad[1] = 0u;
  return p;
}

// the key of candidate k of the home voxel (k = 0: home itself); false: the neighbour's coordinate leaves |v| < 2^20
LOAMX_HD bool loc_candidate_key(uint64_t home, int k, uint64_t& key) {
  key = home;
  if (k == 0) return true;
  const int axis = (k - 1) >> 1;
  const uint32_t shift = 42u - 21u * (uint32_t)axis;
  const uint64_t b = (home >> shift) & 0x1FFFFFull;  // v + 2^20, 1 .. 2^21 - 1
  const uint64_t nb = ((k - 1) & 1) ? b + 1ull : b - 1ull;
  if (nb < 1ull || nb > 0x1FFFFFull) return false;
  key = (home & ~(0x1FFFFFull << shift)) | (nb << shift);
  return true;
}

// steps 1 to 3 of a point: false (counted in n_unused by the caller) when it fails validity or has no cell
LOAMX_HD bool loc_move(const LocRule& R, const double T[7], Vec3 p, Vec3& v, uint64_t& home) {
  if (cloud_validity(p, R.min_r2, R.max_r2) != kCloudUsed) return false;
  v = pose_act(T, p);
  uint32_t u[3];
  return cloud_cell(v, R.leaf, home, u);
}

// step 5: candidate k (in ascending k) against the best so far; best < 0: none yet
LOAMX_HD void loc_offer(Vec3 v, const LocPlane& pl, int k, double& best_d2, int& best, LocPlane& best_plane) {
  if (!pl.usable) return;
  const double dx = v.x - pl.mean[0], dy = v.y - pl.mean[1], dz = v.z - pl.mean[2];
  const double d2 = dx * dx + dy * dy + dz * dz;
  if (best < 0 || d2 < best_d2) best_d2 = d2, best = k, best_plane = pl;
}

struct LocAcc {
  double s[kInfoSums];
  uint32_t c[kLocCounters];
};
LOAMX_HD void loc_acc_clear(LocAcc& A) {
#pragma unroll
  for (int j = 0; j < kInfoSums; j++) A.s[j] = 0.0;
#pragma unroll
  for (int j = 0; j < kLocCounters; j++) A.c[j] = 0u;
}

// steps 6 to 8 of a point that has chosen `pl` (chosen == false: a point without a plane, `pl` is not looked at and nothing is
// counted). Written without a branch around the sums: a row that is absent, gated or not finite is replaced by zeros and added like
// any other (x + 0.0 == x bit for bit: no sum is ever -0.0, they start at +0.0), so that a device build keeps ONE copy of the 28
// sums in registers.
LOAMX_HD void loc_accumulate(const LocRule& R, Vec3 v, const LocPlane& pl, bool chosen, LocAcc& A) {
  loamx_surfel rec;
#pragma unroll
  for (int a = 0; a < 3; a++) rec.mean[a] = pl.mean[a], rec.normal[a] = pl.normal[a];
  const double s = surfel_distance(rec, v);
  const bool gated = chosen && fabs(s) > R.max_distance;
  InfoRow row;
  const Vec3 g = vscale(copysign(1.0, s), v3(pl.normal[0], pl.normal[1], pl.normal[2]));
  const Vec3 vxg = vcross(v, g);
  row.J[0] = vxg.x, row.J[1] = vxg.y, row.J[2] = vxg.z, row.J[3] = g.x, row.J[4] = g.y, row.J[5] = g.z;
  row.r = fabs(s);
  bool finite = (row.r - row.r == 0.0);
#pragma unroll
  for (int j = 0; j < 6; j++) finite = finite && (row.J[j] - row.J[j] == 0.0);
  const bool use = chosen && !gated && finite;
  const bool huber = use && R.huber_delta > 0.0 && row.r > R.huber_delta;
  const double sc = huber ? sqrt(R.huber_delta / row.r) : 1.0;  // (x 1.0 is exact)
#pragma unroll
  for (int j = 0; j < 6; j++) row.J[j] = use ? row.J[j] * sc : 0.0;
  row.r = use ? row.r * sc : 0.0;
  A.c[kLocGated] += gated ? 1u : 0u;
  A.c[kLocUnused] += chosen && !gated && !finite ? 1u : 0u;
  A.c[kLocHuber] += huber ? 1u : 0u;
  A.c[kLocRows] += use ? 1u : 0u;
  int t = 0;
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int j = i; j < 6; j++) A.s[t++] += row.J[i] * row.J[j];
#pragma unroll
  for (int j = 0; j < 6; j++) A.s[21 + j] += row.J[j] * row.r;
  A.s[27] += row.r * row.r;
}

/* ---- the solve ------------------------------------------------------------------------------------------------------------ */
// the state of one cloud between the launches of a call
struct LocState {
  double pose[7];
  double initial_cost, last_rotation, last_translation;
  uint32_t iterations, termination, done, evaluated;
  uint32_t n_rows_initial, pad[3];
};
// the layout of loamx_localize_result (asserted in api_localize.hip)
struct LocResult {
  double pose[7];
  double initial_cost, final_cost, last_rotation, last_translation;
  uint32_t iterations, termination, n_rows, n_huber, n_no_surfel, n_gated, n_unused, used_mask, n_rows_initial, reserved;
};

LOAMX_HD bool loc_finite(double v) { return v - v == 0.0; }

LOAMX_HD void loc_state_init(LocState& S, const double pose[7], uint32_t max_iterations) {
#pragma unroll
  for (int k = 0; k < 7; k++) S.pose[k] = pose[k];
  S.initial_cost = 0.0, S.last_rotation = 0.0, S.last_translation = 0.0;
  S.iterations = 0u, S.termination = kLocMaxIter, S.done = max_iterations == 0u ? 1u : 0u, S.evaluated = 0u;
  S.n_rows_initial = 0u, S.pad[0] = S.pad[1] = S.pad[2] = 0u;
}

// eigenpairs of the sums' triangle; the six bits of the directions with eval[i] > min_eig_per_row n_rows
LOAMX_HD uint32_t loc_eigen(const double sums[kInfoSums], uint32_t n_rows, double min_eig_per_row, double H[36], double eval[6], double evec[36]) {
  info_mirror(sums, H);
  info_eig6(H, eval, evec);
  const double floor_ = min_eig_per_row * (double)n_rows;
  uint32_t mask = 0u;
#pragma unroll
  for (int i = 0; i < 6; i++)
    if (eval[i] > floor_) mask |= 1u << i;
  return mask;
}

// d = - sum over the used directions (ascending i) of evec_i (evec_i . grad) / eval_i
LOAMX_HD void loc_step(const double eval[6], const double evec[36], const double grad[6], uint32_t mask, double d[6]) {
#pragma unroll
  for (int k = 0; k < 6; k++) d[k] = 0.0;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    if (!(mask >> i & 1u)) continue;
    double dot = 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) dot = dot + evec[6 * i + k] * grad[k];
    const double c = dot / eval[i];
#pragma unroll
    for (int k = 0; k < 6; k++) d[k] = d[k] - evec[6 * i + k] * c;
  }
}

// out = (normalise([omega / 2, 1]), t) o T: pgo_retract's arithmetic, applied on the LEFT
LOAMX_HD void loc_retract(const double T[7], const double d[6], double out[7]) {
  const double hx = d[0] / 2.0, hy = d[1] / 2.0, hz = d[2] / 2.0;
  const double n = sqrt(hx * hx + hy * hy + hz * hz + 1.0);
  const double step[7] = {hx / n, hy / n, hz / n, 1.0 / n, d[3], d[4], d[5]};
  pose_compose(step, T, out);
}

// One iteration of a cloud that has not stopped, from the sums of its evaluation at S.pose. The decisions, in this order:
//   0 a non-finite pose -> NOT_FINITE (it can give no row, so it is looked at before the row count)
//   1 n_rows < min_rows -> TOO_FEW_ROWS
//   2 a non-finite step or stepped pose -> NOT_FINITE
//   3 the step is applied, iterations += 1
//   4 |omega| < rot_thresh && |t| < pos_thresh -> CONVERGED
//   5 iterations == max_iterations -> MAX_ITERATIONS
// In 0 to 2 the pose stays.
LOAMX_HD void loc_iterate(LocState& S, const LocSolve& P, const double sums[kInfoSums], uint32_t n_rows) {
  if (!S.evaluated) S.evaluated = 1u, S.initial_cost = sums[27], S.n_rows_initial = n_rows;
  bool pose_ok = true;
#pragma unroll
  for (int k = 0; k < 7; k++) pose_ok = pose_ok && loc_finite(S.pose[k]);
  if (!pose_ok) {
    S.termination = kLocNotFinite, S.done = 1u;
    return;
  }
  if (n_rows < P.min_rows) {
    S.termination = kLocTooFewRows, S.done = 1u;
    return;
  }
  double H[36], eval[6], evec[36], d[6], next[7];
  const uint32_t mask = loc_eigen(sums, n_rows, P.min_eig_per_row, H, eval, evec);
  loc_step(eval, evec, sums + 21, mask, d);
  loc_retract(S.pose, d, next);
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 6; k++) ok = ok && loc_finite(d[k]);
#pragma unroll
  for (int k = 0; k < 7; k++) ok = ok && loc_finite(next[k]);
  if (!ok) {
    S.termination = kLocNotFinite, S.done = 1u;
    return;
  }
#pragma unroll
  for (int k = 0; k < 7; k++) S.pose[k] = next[k];
  S.iterations++;
  S.last_rotation = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  S.last_translation = sqrt(d[3] * d[3] + d[4] * d[4] + d[5] * d[5]);
  if (S.last_rotation < P.rot_thresh && S.last_translation < P.pos_thresh) S.termination = kLocConverged, S.done = 1u;
  else if (S.iterations >= P.max_iterations) S.termination = kLocMaxIter, S.done = 1u;
}

// the last evaluation, at the returned pose: the result record and (info may be null) the information record
LOAMX_HD void loc_finish(const LocState& S, const LocSolve& P, const double sums[kInfoSums], const uint32_t c[kLocCounters], LocResult& out,
                         loamx_reg_information* info) {
  double H[36], eval[6], evec[36];
  const uint32_t mask = loc_eigen(sums, c[kLocRows], P.min_eig_per_row, H, eval, evec);
#pragma unroll
  for (int k = 0; k < 7; k++) out.pose[k] = S.pose[k];
  out.initial_cost = S.evaluated ? S.initial_cost : sums[27];
  out.final_cost = sums[27], out.last_rotation = S.last_rotation, out.last_translation = S.last_translation;
  out.iterations = S.iterations, out.termination = S.termination;
  out.n_rows = c[kLocRows], out.n_huber = c[kLocHuber], out.n_no_surfel = c[kLocNoSurfel], out.n_gated = c[kLocGated], out.n_unused = c[kLocUnused];
  out.used_mask = mask, out.n_rows_initial = S.evaluated ? S.n_rows_initial : c[kLocRows], out.reserved = 0u;
  if (info) {
#pragma unroll
    for (int j = 0; j < 36; j++) info->information[j] = H[j], info->eigenvectors[j] = evec[j];
#pragma unroll
    for (int j = 0; j < 6; j++) info->eigenvalues[j] = eval[j], info->gradient[j] = sums[21 + j];
    info->weighted_sq_error = sums[27];
    // (n_dropped stays 0: the result's n_unused holds the non-finite rows together with the points that had no cell)
    info->n_edge = 0u, info->n_plane = c[kLocRows], info->n_huber = c[kLocHuber], info->n_dropped = 0u;
  }
}

/* ---- the ordered sums: what the accumulate kernel's reduction does to the 256 per-thread values of a chunk ---------------- */
// v[256]: lane l of wavefront w at v[64 w + l]. The shuffle tree 32 .. 1 inside each wavefront, then the four in order.
LOAMX_HD double loc_chunk_sum(double v[kLocThreads]) {
  for (int w = 0; w < kLocThreads / 64; w++)
    for (int off = 32; off >= 1; off >>= 1)
      for (int l = 0; l < off; l++) v[64 * w + l] = v[64 * w + l] + v[64 * w + l + off];
  double s = v[0];
  for (int w = 1; w < kLocThreads / 64; w++) s = s + v[64 * w];
  return s;
}

}  // namespace loamx
