// posegraph_math.h — the pose-graph optimiser (loamx.h: "pose graph"): the error of one edge and its closed-form Jacobians,
// the blocks of the normal equations, the damped 6x6 Cholesky inverse, one row of the block SpMV, the PCG vector update, the
// retraction, the ordered sums and the state machine that decides acceptance, damping and termination.
//
// Everything is FP64, rounded operation by operation (-ffp-contract=off), and uses no libm beyond sqrt: a g++ build of this
// file (tests/hostcheck_posegraph) runs the whole solve in the kernels' orders and is compared with the device by bytes.
// The kernels of posegraph_kernels.hip and that host loop call the same functions; neither restates any arithmetic.
#pragma once
#include "reg_math.h"

namespace loamx {

constexpr uint32_t kPgoChunk = 256;        // items (poses or edges) per chunk of an ordered sum = threads of a workgroup
constexpr double kPgoMinDiagonal = 1e-6;   // Ceres's min_lm_diagonal: the damping of entry k is lambda max(D_kk, this)
constexpr double kPgoMinLambda = 1e-12, kPgoMaxLambda = 1e12;
// loamx.h: LOAMX_PGO_* (api_posegraph.hip asserts the equality)
constexpr uint32_t kPgoCostConverged = 0, kPgoStepConverged = 1, kPgoMaxIterations = 2, kPgoLambdaOverflow = 3, kPgoNothingToDo = 4,
                   kPgoBadInput = 5;

// the layouts of loamx_pgo_edge, loamx_pgo_params, loamx_pgo_summary and loamx_pgo_linearization (asserted in api_posegraph.hip)
struct PgoEdge {
  uint32_t a, b;
  double z[7];
  double info[36];
};
struct PgoParams {
  uint32_t max_iterations, max_pcg_iterations;
  double pcg_tolerance, initial_lambda, cost_tolerance, step_tolerance, huber_delta;
};
struct PgoSummary {
  double initial_cost, final_cost, lambda, max_update;
  uint32_t iterations, accepted, pcg_iterations, termination, n_bad_edges, reserved;
};
struct PgoLinearization {
  double e[6], chi2, weight, A[36], B[36];
};

// what linearisation leaves per edge for the gather and the SpMV (the blocks already carry the Huber weight)
struct PgoEdgeBlocks {
  double Haa[36], Hab[36], Hbb[36], ga[6], gb[6];
};
// what the gather leaves per pose: the damped diagonal block and its inverse (all zeros for a fixed pose or a failed Cholesky)
struct PgoPoseBlocks {
  double D[36], Dinv[36];
};

// PCG iterations the host enqueues per LM iteration: CG ends after as many steps as there are unknowns in exact arithmetic,
// and a truncated solve is still a descent step
LOAMX_HD uint32_t pgo_pcg_cap(uint32_t max_pcg_iterations, uint64_t n_poses) {
  const uint64_t dim = 6 * n_poses;
  return dim < max_pcg_iterations ? (uint32_t)dim : max_pcg_iterations;
}

/* ---- ordered sums ---------------------------------------------------------------------------------------------------
 * A sum over poses or edges: item i contributes v[i % 256] of chunk i / 256 (an absent item 0.0), the chunk is reduced by
 * the tree below (stride 128, 64, ... 1: v[t] += v[t + stride] for t < stride), the chunk results are added in ascending
 * chunk order starting from 0.0. A maximum takes the same walk with max in place of +. */
LOAMX_HD void pgo_tree_add(double* v, uint32_t t, uint32_t stride) {
  if (t < stride) v[t] = v[t] + v[t + stride];
}
LOAMX_HD void pgo_tree_max(double* v, uint32_t t, uint32_t stride) {
  if (t < stride) v[t] = v[t + stride] > v[t] ? v[t + stride] : v[t];
}
LOAMX_HD double pgo_sum_chunks(const double* part, uint32_t n_chunks) {
  double s = 0.0;
  for (uint32_t c = 0; c < n_chunks; c++) s = s + part[c];
  return s;
}
LOAMX_HD double pgo_max_chunks(const double* part, uint32_t n_chunks) {
  double s = 0.0;
  for (uint32_t c = 0; c < n_chunks; c++) s = part[c] > s ? part[c] : s;
  return s;
}

/* ---- the error of an edge ---------------------------------------------------------------------------------------------- */
LOAMX_HD void pgo_pose_inverse(const double T[7], double out[7]) {
  out[0] = -T[0], out[1] = -T[1], out[2] = -T[2], out[3] = T[3];
  const Vec3 r = quat_rotate(out, v3(T[4], T[5], T[6]));
  out[4] = -r.x, out[5] = -r.y, out[6] = -r.z;
}
LOAMX_HD double pgo_info_at(const double* info, int i, int j) { return i <= j ? info[6 * i + j] : info[6 * j + i]; }

struct PgoError {
  double zhat[7];  // T_a^-1 o T_b
  double qd[4];    // q_zhat (x) conj(q_Z)
  double td[3];    // t_zhat - R_D t_Z
  double sgn;      // +1, or -1 when w_D < 0
  double e[6];
};
LOAMX_HD void pgo_error(const double Ta[7], const double Tb[7], const double Z[7], PgoError& E) {
  double inv[7];
  pgo_pose_inverse(Ta, inv);
  pose_compose(inv, Tb, E.zhat);
  const double zc[4] = {-Z[0], -Z[1], -Z[2], Z[3]};
  quat_mul(E.zhat, zc, E.qd);
  const Vec3 rt = quat_rotate(E.qd, v3(Z[4], Z[5], Z[6]));
  E.td[0] = E.zhat[4] - rt.x, E.td[1] = E.zhat[5] - rt.y, E.td[2] = E.zhat[6] - rt.z;
  E.sgn = E.qd[3] < 0.0 ? -1.0 : 1.0;
  const double s2 = 2.0 * E.sgn;
  E.e[0] = s2 * E.qd[0], E.e[1] = s2 * E.qd[1], E.e[2] = s2 * E.qd[2];
  E.e[3] = E.td[0], E.e[4] = E.td[1], E.e[5] = E.td[2];
}
// chi2 = e^T Omega e through Oe = Omega e (row by row, columns ascending), then e . Oe (ascending)
LOAMX_HD double pgo_chi2(const double* info, const double e[6], double Oe[6]) {
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 6; j++) s = s + pgo_info_at(info, i, j) * e[j];
    Oe[i] = s;
  }
  double c = 0.0;
#pragma unroll
  for (int i = 0; i < 6; i++) c = c + e[i] * Oe[i];
  return c;
}
// Huber: the weight of the edge's blocks and gradients, and its cost
LOAMX_HD double pgo_weight(double chi2, double huber_delta, double& cost) {
  if (huber_delta > 0.0 && chi2 > huber_delta * huber_delta) {
    const double chi = sqrt(chi2);
    cost = (2.0 * huber_delta) * chi - huber_delta * huber_delta;
    return huber_delta / chi;
  }
  cost = chi2;
  return 1.0;
}
// the cost of an edge alone (the evaluation at a candidate)
LOAMX_HD double pgo_edge_cost(const double Ta[7], const double Tb[7], const PgoEdge& ed, double huber_delta) {
  PgoError E;
  double Oe[6], cost;
  pgo_error(Ta, Tb, ed.z, E);
  (void)pgo_weight(pgo_chi2(ed.info, E.e, Oe), huber_delta, cost);
  return cost;
}

/* ---- Jacobians: A = de/d delta_a, B = de/d delta_b at delta = 0 for T_i <- T_i o (normalise([omega_i / 2, 1]), tau_i) ----
 * a: zhat' = Delta^-1 o zhat, so q_D' = q_D - [omega/2, 0] (x) q_D and t_D' = R_delta^T (t_D - tau):
 *      A = [ -s vec(E_k (x) q_D)  0 ;  [t_D]x  -I ]
 * b: zhat' = zhat o Delta, so q_D' = q_D + q_zhat (x) [omega/2, 0] (x) conj(q_Z), t_D' = t_zhat + R_zhat tau - R_zhat R_delta u
 *    with u = R_Z^T t_Z:
 *      B = [ s vec(q_zhat (x) E_k (x) conj(q_Z))  0 ;  R_zhat [u]x  R_zhat ]
 * (E_k the pure unit quaternion of axis k, s = sgn(w_D); the normalisation of [omega/2, 1] has no first-order term.)
 * Row-major 6 x 6, columns 0-2 omega, 3-5 tau. */
LOAMX_HD void pgo_jacobians(const PgoError& E, const double Z[7], double A[36], double B[36]) {
#pragma unroll
  for (int i = 0; i < 36; i++) A[i] = 0.0, B[i] = 0.0;
  const double zc[4] = {-Z[0], -Z[1], -Z[2], Z[3]};
  const Vec3 u = quat_rotate(zc, v3(Z[4], Z[5], Z[6]));
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double ek[4] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0, 0.0};
    const Vec3 axis = v3(ek[0], ek[1], ek[2]);
    double qa[4], qb0[4], qb[4];
    quat_mul(ek, E.qd, qa);
    quat_mul(E.zhat, ek, qb0);
    quat_mul(qb0, zc, qb);
    const Vec3 ta = vcross(v3(E.td[0], E.td[1], E.td[2]), axis);  // column k of [t_D]x
    const Vec3 tb = quat_rotate(E.zhat, vcross(u, axis));         // column k of R_zhat [u]x
    const Vec3 rk = quat_rotate(E.zhat, axis);                    // column k of R_zhat
    A[0 * 6 + k] = -(E.sgn * qa[0]), A[1 * 6 + k] = -(E.sgn * qa[1]), A[2 * 6 + k] = -(E.sgn * qa[2]);
    A[3 * 6 + k] = ta.x, A[4 * 6 + k] = ta.y, A[5 * 6 + k] = ta.z;
    A[(3 + k) * 6 + 3 + k] = -1.0;
    B[0 * 6 + k] = E.sgn * qb[0], B[1 * 6 + k] = E.sgn * qb[1], B[2 * 6 + k] = E.sgn * qb[2];
    B[3 * 6 + k] = tb.x, B[4 * 6 + k] = tb.y, B[5 * 6 + k] = tb.z;
    B[3 * 6 + 3 + k] = rk.x, B[4 * 6 + 3 + k] = rk.y, B[5 * 6 + 3 + k] = rk.z;
  }
}

// out = w X^T (Omega Y) with OY = Omega Y given (every sum ascending in its index)
LOAMX_HD void pgo_xt_oy(const double X[36], const double OY[36], double w, double out[36]) {
#pragma unroll
  for (int i = 0; i < 6; i++) {
#pragma unroll
    for (int j = 0; j < 6; j++) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 6; k++) s = s + X[6 * k + i] * OY[6 * k + j];
      out[6 * i + j] = w * s;
    }
  }
}
LOAMX_HD void pgo_omega_times(const double* info, const double Y[36], double OY[36]) {
#pragma unroll
  for (int i = 0; i < 6; i++) {
#pragma unroll
    for (int j = 0; j < 6; j++) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 6; k++) s = s + pgo_info_at(info, i, k) * Y[6 * k + j];
      OY[6 * i + j] = s;
    }
  }
}

// One edge at the poses of its ends: the record of loamx_pose_graph_linearize (lin, may be null), the blocks (blk, may be
// null) and the return value, the edge's cost.
LOAMX_HD double pgo_linearize_edge(const double Ta[7], const double Tb[7], const PgoEdge& ed, double huber_delta, PgoLinearization* lin,
                                   PgoEdgeBlocks* blk) {
  PgoError E;
  double Oe[6], cost, A[36], B[36], OY[36];
  pgo_error(Ta, Tb, ed.z, E);
  const double chi2 = pgo_chi2(ed.info, E.e, Oe);
  const double w = pgo_weight(chi2, huber_delta, cost);
  pgo_jacobians(E, ed.z, A, B);
  if (lin) {
#pragma unroll
    for (int i = 0; i < 6; i++) lin->e[i] = E.e[i];
    lin->chi2 = chi2, lin->weight = w;
#pragma unroll
    for (int i = 0; i < 36; i++) lin->A[i] = A[i], lin->B[i] = B[i];
  }
  if (blk) {
#pragma unroll
    for (int i = 0; i < 6; i++) {
      double sa = 0.0, sb = 0.0;
#pragma unroll
      for (int k = 0; k < 6; k++) sa = sa + A[6 * k + i] * Oe[k], sb = sb + B[6 * k + i] * Oe[k];
      blk->ga[i] = w * sa, blk->gb[i] = w * sb;
    }
    pgo_omega_times(ed.info, A, OY);
    pgo_xt_oy(A, OY, w, blk->Haa);
    pgo_omega_times(ed.info, B, OY);
    pgo_xt_oy(A, OY, w, blk->Hab);
    pgo_xt_oy(B, OY, w, blk->Hbb);
  }
  return cost;
}

/* ---- incidence -----------------------------------------------------------------------------------------------------------
 * entry = 2 edge + side (side 0: the pose is the edge's a, 1: its b); a pose's entries stand ascending. */
LOAMX_HD bool pgo_edge_ok(uint32_t a, uint32_t b, uint64_t n_poses) { return a != b && a < n_poses && b < n_poses; }
// in-place heap sort of a pose's segment (the fill leaves it in any order; the entries are distinct)
LOAMX_HD void pgo_sort_segment(uint32_t* v, uint32_t n) {
  if (n < 2) return;
  for (uint32_t start = n / 2; start-- > 0;) {
    uint32_t root = start;
    for (;;) {
      uint32_t child = 2 * root + 1;
      if (child >= n) break;
      if (child + 1 < n && v[child] < v[child + 1]) child++;
      if (v[root] >= v[child]) break;
      const uint32_t t = v[root];
      v[root] = v[child], v[child] = t, root = child;
    }
  }
  for (uint32_t end = n - 1; end > 0; end--) {
    const uint32_t t0 = v[0];
    v[0] = v[end], v[end] = t0;
    uint32_t root = 0;
    for (;;) {
      uint32_t child = 2 * root + 1;
      if (child >= end) break;
      if (child + 1 < end && v[child] < v[child + 1]) child++;
      if (v[root] >= v[child]) break;
      const uint32_t t = v[root];
      v[root] = v[child], v[child] = t, root = child;
    }
  }
}

/* ---- gather: the pose's diagonal block and gradient, damping, Cholesky inverse ------------------------------------------- */
// inv = (L L^T)^-1 of the symmetric M (lower triangle read); false (inv all zeros) when a pivot is not positive
LOAMX_HD bool pgo_cholesky_inverse(const double M[36], double inv[36]) {
  double L[36], Li[36];
#pragma unroll
  for (int i = 0; i < 36; i++) L[i] = 0.0, Li[i] = 0.0, inv[i] = 0.0;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; j++) {
    double d = M[6 * j + j];
#pragma unroll
    for (int k = 0; k < j; k++) d = d - L[6 * j + k] * L[6 * j + k];
    if (!(d > 0.0)) ok = false;
    const double ljj = sqrt(d);
    L[6 * j + j] = ljj;
#pragma unroll
    for (int i = j + 1; i < 6; i++) {
      double s = M[6 * i + j];
#pragma unroll
      for (int k = 0; k < j; k++) s = s - L[6 * i + k] * L[6 * j + k];
      L[6 * i + j] = s / ljj;
    }
  }
  if (!ok) return false;
  // Li = L^-1 (lower), column by column
#pragma unroll
  for (int c = 0; c < 6; c++) {
#pragma unroll
    for (int i = c; i < 6; i++) {
      double s = i == c ? 1.0 : 0.0;
#pragma unroll
      for (int k = c; k < i; k++) s = s - L[6 * i + k] * Li[6 * k + c];
      Li[6 * i + c] = s / L[6 * i + i];
    }
  }
#pragma unroll
  for (int i = 0; i < 6; i++) {
#pragma unroll
    for (int j = i; j < 6; j++) {
      double s = 0.0;
#pragma unroll
      for (int k = j; k < 6; k++) s = s + Li[6 * k + i] * Li[6 * k + j];
      inv[6 * i + j] = s, inv[6 * j + i] = s;
    }
  }
  return true;
}
LOAMX_HD void pgo_mat_vec(const double M[36], const double v[6], double out[6]) {
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 6; j++) s = s + M[6 * i + j] * v[j];
    out[i] = s;
  }
}
LOAMX_HD void pgo_mat_t_vec(const double M[36], const double v[6], double out[6]) {
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 6; j++) s = s + M[6 * j + i] * v[j];
    out[i] = s;
  }
}
LOAMX_HD double pgo_dot6(const double a[6], const double b[6]) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 6; i++) s = s + a[i] * b[i];
  return s;
}

// Pose i at the start of an LM iteration: its blocks, x = 0, r = -g, z = Dinv r (p of the first PCG iteration is z);
// returns the pose's share of r.z. `list`: the pose's `deg` incidence entries. A fixed pose has all of it zero.
LOAMX_HD double pgo_gather_pose(bool fixed, const uint32_t* list, uint32_t deg, const PgoEdgeBlocks* blocks, double lambda, PgoPoseBlocks& pb,
                                double x[6], double r[6], double z[6]) {
  double D[36], g[6];
#pragma unroll
  for (int i = 0; i < 36; i++) D[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 6; i++) g[i] = 0.0, x[i] = 0.0;
  if (!fixed) {
    for (uint32_t k = 0; k < deg; k++) {
      const uint32_t ent = list[k];
      const PgoEdgeBlocks& b = blocks[ent >> 1];
      const double* H = (ent & 1u) ? b.Hbb : b.Haa;
      const double* gg = (ent & 1u) ? b.gb : b.ga;
#pragma unroll
      for (int i = 0; i < 36; i++) D[i] = D[i] + H[i];
#pragma unroll
      for (int i = 0; i < 6; i++) g[i] = g[i] + gg[i];
    }
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const double d = D[7 * k];
      D[7 * k] = d + lambda * (d > kPgoMinDiagonal ? d : kPgoMinDiagonal);
    }
  }
  const bool ok = !fixed && pgo_cholesky_inverse(D, pb.Dinv);
  if (!ok) {
#pragma unroll
    for (int i = 0; i < 36; i++) D[i] = 0.0, pb.Dinv[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) g[i] = 0.0;
  }
#pragma unroll
  for (int i = 0; i < 36; i++) pb.D[i] = D[i];
#pragma unroll
  for (int i = 0; i < 6; i++) r[i] = -g[i];
  pgo_mat_vec(pb.Dinv, r, z);
  return pgo_dot6(r, z);
}

// out of the system: fixed, or its Cholesky failed (the inverse of a positive definite block has a positive corner)
LOAMX_HD bool pgo_pose_dead(bool fixed, const PgoPoseBlocks& pb) { return fixed || pb.Dinv[0] == 0.0; }

/* ---- one row of the block SpMV --------------------------------------------------------------------------------------------
 * p_j = z_j (first PCG iteration) or z_j + beta p_old_j, formed where it is read: the row of pose i writes p_i and forms its
 * neighbours' p on the fly from the same two arrays, so the direction update needs no pass of its own. */
LOAMX_HD void pgo_direction(const double* z, const double* p_old, uint32_t j, bool first, double beta, double p[6]) {
#pragma unroll
  for (int k = 0; k < 6; k++) p[k] = first ? z[6 * (size_t)j + k] : z[6 * (size_t)j + k] + beta * p_old[6 * (size_t)j + k];
}
// q_i = D_i p_i + sum over the incidence list (H_ab p_b for side 0, H_ab^T p_a for side 1; neighbours that are fixed are
// skipped), in list order; writes p_i, q_i; returns p_i . q_i. `dead`: the pose is out of the system (fixed, failed Cholesky).
LOAMX_HD double pgo_spmv_row(uint32_t i, bool dead, const uint8_t* fixed, const uint32_t* list, uint32_t deg, const PgoEdge* edges,
                             const PgoEdgeBlocks* blocks, const PgoPoseBlocks& pb, const double* z, const double* p_old, bool first, double beta,
                             double* p_new, double* q) {
  double p[6], acc[6], t[6], pj[6];
  if (dead) {
#pragma unroll
    for (int k = 0; k < 6; k++) p_new[6 * (size_t)i + k] = 0.0, q[6 * (size_t)i + k] = 0.0;
    return 0.0;
  }
  pgo_direction(z, p_old, i, first, beta, p);
  pgo_mat_vec(pb.D, p, acc);
  for (uint32_t k = 0; k < deg; k++) {
    const uint32_t ent = list[k], e = ent >> 1;
    const uint32_t j = (ent & 1u) ? edges[e].a : edges[e].b;
    if (fixed[j]) continue;
    pgo_direction(z, p_old, j, first, beta, pj);
    if (ent & 1u) pgo_mat_t_vec(blocks[e].Hab, pj, t);
    else pgo_mat_vec(blocks[e].Hab, pj, t);
#pragma unroll
    for (int c = 0; c < 6; c++) acc[c] = acc[c] + t[c];
  }
#pragma unroll
  for (int k = 0; k < 6; k++) p_new[6 * (size_t)i + k] = p[k], q[6 * (size_t)i + k] = acc[k];
  return pgo_dot6(p, acc);
}
// x += alpha p, r -= alpha q, z = Dinv r; returns r . z
LOAMX_HD double pgo_update_pose(uint32_t i, const PgoPoseBlocks& pb, double alpha, const double* p, const double* q, double* x, double* r, double* z) {
  double rr[6], zz[6];
#pragma unroll
  for (int k = 0; k < 6; k++) {
    x[6 * (size_t)i + k] = x[6 * (size_t)i + k] + alpha * p[6 * (size_t)i + k];
    rr[k] = r[6 * (size_t)i + k] - alpha * q[6 * (size_t)i + k];
  }
  pgo_mat_vec(pb.Dinv, rr, zz);
#pragma unroll
  for (int k = 0; k < 6; k++) r[6 * (size_t)i + k] = rr[k], z[6 * (size_t)i + k] = zz[k];
  return pgo_dot6(rr, zz);
}

/* ---- retraction ------------------------------------------------------------------------------------------------------------ */
// out = T o (normalise([omega / 2, 1]), tau); returns max |delta_k|. A fixed pose is copied.
LOAMX_HD double pgo_retract(bool fixed, const double T[7], const double d[6], double out[7]) {
  if (fixed) {
#pragma unroll
    for (int k = 0; k < 7; k++) out[k] = T[k];
    return 0.0;
  }
  const double hx = d[0] / 2.0, hy = d[1] / 2.0, hz = d[2] / 2.0;
  const double n = sqrt(hx * hx + hy * hy + hz * hz + 1.0);
  const double step[7] = {hx / n, hy / n, hz / n, 1.0 / n, d[3], d[4], d[5]};
  pose_compose(T, step, out);
  double m = 0.0;
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const double a = d[k] < 0.0 ? -d[k] : d[k];
    m = a > m ? a : m;
  }
  return m;
}

/* ---- the state of a solve: one record, every kernel that changes it reads one copy and writes the other ------------------ */
struct PgoState {
  double lambda, cost, initial_cost, max_update;
  double rz, rz0;          // r.z of the current PCG iterate and of the first
  double beta, alpha;      // of the PCG iteration under way
  uint32_t iterations, accepted, pcg_total, termination, n_bad;
  uint32_t done;           // the solve has terminated: every later launch returns at once
  uint32_t pcg_done, pcg_it;  // the inner solve of this LM iteration has stopped; its iterations so far
};
LOAMX_HD void pgo_state_init(PgoState& s, const PgoParams& P) {
  s.lambda = P.initial_lambda, s.cost = 0.0, s.initial_cost = 0.0, s.max_update = 0.0;
  s.rz = 0.0, s.rz0 = 0.0, s.beta = 0.0, s.alpha = 0.0;
  s.iterations = 0, s.accepted = 0, s.pcg_total = 0, s.termination = kPgoMaxIterations, s.n_bad = 0;
  s.done = 0, s.pcg_done = 0, s.pcg_it = 0;
}
// behind the incidence counts: refusals and empty problems
LOAMX_HD void pgo_state_counts(PgoState& s, uint32_t n_bad, uint64_t n_edges, uint64_t n_free) {
  s.n_bad = n_bad;
  if (n_bad) s.termination = kPgoBadInput, s.done = 1;
  else if (n_edges == 0 || n_free == 0) s.termination = kPgoNothingToDo, s.done = 1;
}
// gather: the cost at the current poses (the sum of the linearisation's chunk partials)
LOAMX_HD void pgo_state_gather(PgoState& s, double cost) {
  s.cost = cost;
  if (s.iterations == 0) s.initial_cost = cost;
  s.pcg_done = 0, s.pcg_it = 0;
}
// SpMV prologue: rz = the sum of the r.z partials. The inner solve stops here at rz <= tol^2 rz0.
LOAMX_HD void pgo_state_spmv(PgoState& s, double rz, double pcg_tolerance) {
  if (s.pcg_it == 0) s.rz0 = rz, s.beta = 0.0;
  else s.beta = rz / s.rz;
  s.rz = rz;
  if (!(rz > pcg_tolerance * pcg_tolerance * s.rz0)) s.pcg_done = 1;
}
// update prologue: pq = the sum of the p.q partials. p.q <= 0 stops the inner solve and keeps x.
LOAMX_HD void pgo_state_update(PgoState& s, double pq, uint32_t pcg_cap) {
  if (!(pq > 0.0)) {
    s.pcg_done = 1;
    return;
  }
  s.alpha = s.rz / pq;
  s.pcg_it++, s.pcg_total++;
  if (s.pcg_it >= pcg_cap) s.pcg_done = 2;  // (this update still runs; no SpMV follows it)
}
// decide: c1 = the cost at the candidate, mx = max |delta|. Returns true when the candidate becomes the poses.
LOAMX_HD bool pgo_state_decide(PgoState& s, const PgoParams& P, double c1, double mx) {
  bool accept = false;
  s.iterations++;
  s.max_update = mx;
  if (mx <= P.step_tolerance) {
    s.termination = kPgoStepConverged, s.done = 1;
  } else if (c1 < s.cost) {
    accept = true;
    s.accepted++;
    const double l = s.lambda / 10.0;
    s.lambda = l > kPgoMinLambda ? l : kPgoMinLambda;
    if (s.cost - c1 <= P.cost_tolerance * s.cost) s.termination = kPgoCostConverged, s.done = 1;
    s.cost = c1;
  } else {
    s.lambda = 10.0 * s.lambda;
    if (s.lambda > kPgoMaxLambda) s.termination = kPgoLambdaOverflow, s.done = 1;
  }
  if (!s.done && s.iterations >= P.max_iterations) s.termination = kPgoMaxIterations, s.done = 1;
  return accept;
}
LOAMX_HD void pgo_state_summary(const PgoState& s, PgoSummary& out) {
  out.initial_cost = s.initial_cost, out.final_cost = s.cost, out.lambda = s.lambda, out.max_update = s.max_update;
  out.iterations = s.iterations, out.accepted = s.accepted, out.pcg_iterations = s.pcg_total, out.termination = s.termination;
  out.n_bad_edges = s.n_bad, out.reserved = 0;
}

}  // namespace loamx
