// TEST-ONLY: posegraph_math.h (the pose-graph optimiser's arithmetic) compiled for the host behind extern "C" wrappers, with a
// host loop that runs the whole solve in the kernels' orders: one loop per kernel of posegraph_kernels.hip, the same header
// functions per item, the same chunks of 256, the same tree, the same state machine. tests/test_posegraph_hostcheck.py checks
// it against a numpy model and an independent solver; tests/test_gpu_posegraph.py compares the device with it by bytes. With
// -DHOSTCHECK_POSEGRAPH_MAIN the file is a stand-alone program that runs the same wrappers over generated graphs (the `san`
// target builds it with -fsanitize=address,undefined).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../loam_amd/csrc/posegraph_math.h"

using namespace loamx;

namespace {

double chunk_sum(const std::vector<double>& vals, bool take_max, std::vector<double>& part) {
  const size_t n = vals.size(), nc = (n + kPgoChunk - 1) / kPgoChunk;
  part.assign(nc, 0.0);
  for (size_t c = 0; c < nc; c++) {
    double v[kPgoChunk];
    for (uint32_t t = 0; t < kPgoChunk; t++) v[t] = c * kPgoChunk + t < n ? vals[c * kPgoChunk + t] : 0.0;
    for (uint32_t s = kPgoChunk / 2; s > 0; s >>= 1)
      for (uint32_t t = 0; t < s; t++) take_max ? pgo_tree_max(v, t, s) : pgo_tree_add(v, t, s);
    part[c] = v[0];
  }
  return take_max ? pgo_max_chunks(part.data(), (uint32_t)nc) : pgo_sum_chunks(part.data(), (uint32_t)nc);
}

}  // namespace

extern "C" {

uint64_t hostcheck_pgo_sizes(uint64_t* out) {
  out[0] = sizeof(PgoEdge), out[1] = sizeof(PgoParams), out[2] = sizeof(PgoSummary), out[3] = sizeof(PgoLinearization);
  return 4;
}

// e, chi2, weight, A, B of every edge (the caller has checked the indices)
void hostcheck_pgo_linearize(const double* poses, const PgoEdge* edges, uint64_t n_edges, double huber_delta, PgoLinearization* out) {
  for (uint64_t e = 0; e < n_edges; e++)
    (void)pgo_linearize_edge(poses + 7 * (size_t)edges[e].a, poses + 7 * (size_t)edges[e].b, edges[e], huber_delta, out + e, nullptr);
}

// out = T o (normalise([omega / 2, 1]), tau)
void hostcheck_pgo_retract(const double* T, const double* delta, double* out) { (void)pgo_retract(false, T, delta, out); }

// returns 0 when M has a Cholesky factor; inv = its inverse
int hostcheck_pgo_cholesky_inverse(const double* M, double* inv) { return pgo_cholesky_inverse(M, inv) ? 0 : 1; }

void hostcheck_pgo_sort(uint32_t* v, uint32_t n) { pgo_sort_segment(v, n); }

// the whole solve as loamx_pose_graph_optimize_dev enqueues it; fixed may be null (pose 0 only)
void hostcheck_pgo_optimize(double* poses, uint64_t n_poses, const uint8_t* fixed_in, const PgoEdge* edges, uint64_t n_edges, const PgoParams* Pp,
                            PgoSummary* summary) {
  const PgoParams P = *Pp;
  PgoState s;
  pgo_state_init(s, P);
  if (n_poses == 0 || n_edges == 0) {
    pgo_state_counts(s, 0u, 0u, 0u);
    pgo_state_summary(s, *summary);
    return;
  }
  // degree kernel
  std::vector<uint8_t> fixed(n_poses);
  std::vector<uint32_t> deg(n_poses, 0u);
  uint32_t n_bad = 0;
  for (uint64_t i = 0; i < n_poses; i++) fixed[i] = fixed_in ? (fixed_in[i] != 0) : (i == 0);
  for (uint64_t e = 0; e < n_edges; e++) {
    if (pgo_edge_ok(edges[e].a, edges[e].b, n_poses)) deg[edges[e].a]++, deg[edges[e].b]++;
    else n_bad++;
  }
  // scan kernel
  std::vector<uint32_t> off(n_poses + 1, 0u), cursor(n_poses, 0u);
  uint64_t n_free = 0;
  if (!n_bad) {
    for (uint64_t i = 0; i < n_poses; i++) off[i + 1] = off[i] + deg[i], cursor[i] = off[i], n_free += fixed[i] ? 0 : 1;
  }
  pgo_state_counts(s, n_bad, n_edges, n_free);
  // fill (here from the last edge down, so that the sort has work) and sort kernels
  std::vector<uint32_t> list(2 * n_edges, 0u);
  if (!s.done) {
    for (uint64_t e = n_edges; e-- > 0;) {
      list[cursor[edges[e].a]++] = (uint32_t)(2 * e);
      list[cursor[edges[e].b]++] = (uint32_t)(2 * e + 1);
    }
    for (uint64_t i = 0; i < n_poses; i++) pgo_sort_segment(list.data() + off[i], off[i + 1] - off[i]);
  }
  std::vector<PgoEdgeBlocks> blocks(n_edges);
  std::vector<PgoPoseBlocks> pb(n_poses);
  std::vector<double> x(6 * n_poses), r(6 * n_poses), z(6 * n_poses), q(6 * n_poses), p[2];
  p[0].assign(6 * n_poses, 0.0), p[1].assign(6 * n_poses, 0.0);
  std::vector<double> cand(7 * n_poses), per_edge(n_edges), per_pose(n_poses), part, part2;
  const uint32_t cap = pgo_pcg_cap(P.max_pcg_iterations, n_poses);
  for (uint32_t it = 0; it < P.max_iterations && !s.done; it++) {
    // linearise + gather
    for (uint64_t e = 0; e < n_edges; e++)
      per_edge[e] = pgo_linearize_edge(poses + 7 * (size_t)edges[e].a, poses + 7 * (size_t)edges[e].b, edges[e], P.huber_delta, nullptr, &blocks[e]);
    pgo_state_gather(s, chunk_sum(per_edge, false, part));
    for (uint64_t i = 0; i < n_poses; i++)
      per_pose[i] = pgo_gather_pose(fixed[i] != 0, list.data() + off[i], off[i + 1] - off[i], blocks.data(), s.lambda, pb[i], &x[6 * i], &r[6 * i], &z[6 * i]);
    double rz = chunk_sum(per_pose, false, part);
    for (uint32_t j = 0; j < cap && !s.pcg_done; j++) {
      // SpMV kernel
      const bool first = s.pcg_it == 0;
      pgo_state_spmv(s, rz, P.pcg_tolerance);
      if (s.pcg_done) break;
      for (uint64_t i = 0; i < n_poses; i++)
        per_pose[i] = pgo_spmv_row((uint32_t)i, pgo_pose_dead(fixed[i] != 0, pb[i]), fixed.data(), list.data() + off[i], off[i + 1] - off[i], edges,
                                   blocks.data(), pb[i], z.data(), p[j & 1].data(), first, s.beta, p[(j & 1) ^ 1].data(), q.data());
      const double pq = chunk_sum(per_pose, false, part);
      // update kernel
      pgo_state_update(s, pq, cap);
      if (s.pcg_done == 1) break;
      for (uint64_t i = 0; i < n_poses; i++)
        per_pose[i] = pgo_update_pose((uint32_t)i, pb[i], s.alpha, p[(j & 1) ^ 1].data(), q.data(), x.data(), r.data(), z.data());
      rz = chunk_sum(per_pose, false, part);
    }
    // candidate, its cost, the decision
    for (uint64_t i = 0; i < n_poses; i++) per_pose[i] = pgo_retract(fixed[i] != 0, poses + 7 * i, &x[6 * i], &cand[7 * i]);
    const double mx = chunk_sum(per_pose, true, part);
    for (uint64_t e = 0; e < n_edges; e++)
      per_edge[e] = pgo_edge_cost(cand.data() + 7 * (size_t)edges[e].a, cand.data() + 7 * (size_t)edges[e].b, edges[e], P.huber_delta);
    const double c1 = chunk_sum(per_edge, false, part2);
    if (pgo_state_decide(s, P, c1, mx)) memcpy(poses, cand.data(), 7 * n_poses * sizeof(double));
  }
  pgo_state_summary(s, *summary);
}

}  // extern "C"

#ifdef HOSTCHECK_POSEGRAPH_MAIN
#include <math.h>
int main() {
  uint64_t state = 88172645463325252ull;
  auto rnd = [&]() {
    state ^= state << 13, state ^= state >> 7, state ^= state << 17;
    return (double)(state >> 11) / 9007199254740992.0;
  };
  const uint64_t sizes[5] = {2, 3, 12, 100, 257};
  for (uint64_t n : sizes) {
    // truth: a ring; measurements composed from it; the start drifts away from it
    std::vector<double> truth(7 * n), poses(7 * n);
    for (uint64_t i = 0; i < n; i++) {
      const double th = 6.283185307179586 * (double)i / (double)n, h = th / 2.0;
      const double T[7] = {0.0, 0.0, sin(h), cos(h), 10.0 * cos(th), 10.0 * sin(th), 0.1 * rnd()};
      for (int k = 0; k < 7; k++) truth[7 * i + k] = T[k];
    }
    std::vector<PgoEdge> edges;
    auto add = [&](uint32_t a, uint32_t b) {
      PgoEdge e;
      memset(&e, 0, sizeof(e));
      e.a = a, e.b = b;
      double inv[7];
      pgo_pose_inverse(&truth[7 * a], inv);
      pose_compose(inv, &truth[7 * b], e.z);
      for (int k = 0; k < 6; k++) e.info[7 * k] = k < 3 ? 400.0 : 100.0;
      edges.push_back(e);
    };
    for (uint32_t i = 0; i + 1 < n; i++) add(i, i + 1);
    if (n > 2) add((uint32_t)n - 1, 0);
    for (uint32_t i = 0; i + 7 < n; i += 5) add(i + 7, i);  // listed with b < a
    for (int k = 0; k < 7; k++) poses[k] = truth[k];
    for (uint64_t i = 1; i < n; i++) {
      const double d[6] = {0.002 * (rnd() - 0.5), 0.002 * (rnd() - 0.5), 0.01 * (rnd() - 0.5), 0.05 * (rnd() - 0.5), 0.05 * (rnd() - 0.5), 0.01 * (rnd() - 0.5)};
      double inv[7], step[7], moved[7];
      pgo_pose_inverse(&truth[7 * (i - 1)], inv);
      pose_compose(inv, &truth[7 * i], step);
      pose_compose(&poses[7 * (i - 1)], step, moved);
      hostcheck_pgo_retract(moved, d, &poses[7 * i]);
    }
    PgoParams P = {20, 500, 1e-8, 1e-4, 1e-9, 1e-10, 0.0};
    PgoSummary S;
    std::vector<PgoLinearization> lin(edges.size());
    hostcheck_pgo_linearize(poses.data(), edges.data(), edges.size(), 1.0, lin.data());
    hostcheck_pgo_optimize(poses.data(), n, nullptr, edges.data(), edges.size(), &P, &S);
    if (!(S.final_cost <= S.initial_cost) || S.termination > kPgoLambdaOverflow || !(S.final_cost < 1e-6 * (1.0 + S.initial_cost)))
      return printf("n %llu: cost %g -> %g, termination %u\n", (unsigned long long)n, S.initial_cost, S.final_cost, S.termination), 1;
    for (uint64_t i = 0; i < 7 * n; i++)
      if (!isfinite(poses[i])) return printf("n %llu: a pose is not finite\n", (unsigned long long)n), 1;
    // the routes around the inner solve: caps of either parity with further iterations, Huber weights, a rejected step (the
    // start thrown far off), and information that is not positive semi-definite (p.q <= 0, or a pose block without a Cholesky
    // factor)
    for (int route = 0; route < 6; route++) {
      std::vector<double> work = poses;
      std::vector<PgoEdge> ed = edges;
      PgoParams Q = P;
      Q.max_iterations = 4;
      if (route == 0) Q.max_pcg_iterations = 1;
      if (route == 1) Q.max_pcg_iterations = 3;
      if (route == 2) Q.huber_delta = 0.5;
      if (route >= 2)
        for (uint64_t i = 1; i < n; i++) {
          const double d[6] = {1.5 * (rnd() - 0.5), 1.5 * (rnd() - 0.5), 1.5 * (rnd() - 0.5), 3.0 * (rnd() - 0.5), 3.0 * (rnd() - 0.5), 3.0 * (rnd() - 0.5)};
          double moved[7];
          hostcheck_pgo_retract(&work[7 * i], d, moved);
          for (int k = 0; k < 7; k++) work[7 * i + k] = moved[k];
        }
      if (route >= 4)
        for (int k = 0; k < 36; k++) ed.back().info[k] *= route == 4 ? -0.2 : -2.0;
      hostcheck_pgo_optimize(work.data(), n, nullptr, ed.data(), ed.size(), &Q, &S);
      if (S.termination > kPgoLambdaOverflow || !(S.final_cost <= S.initial_cost) || S.iterations == 0)
        return printf("n %llu route %d: cost %g -> %g, termination %u\n", (unsigned long long)n, route, S.initial_cost, S.final_cost, S.termination), 1;
      for (uint64_t i = 0; i < 7 * n; i++)
        if (!isfinite(work[i])) return printf("n %llu route %d: a pose is not finite\n", (unsigned long long)n, route), 1;
    }
    // a bad edge is counted and never followed
    edges[0].b = (uint32_t)n + 5;
    std::vector<double> before = poses;
    hostcheck_pgo_optimize(poses.data(), n, nullptr, edges.data(), edges.size(), &P, &S);
    if (S.termination != kPgoBadInput || S.n_bad_edges != 1 || memcmp(before.data(), poses.data(), 7 * n * sizeof(double)) != 0)
      return printf("n %llu: bad edge not refused\n", (unsigned long long)n), 1;
  }
  printf("hostcheck_posegraph ok\n");
  return 0;
}
#endif
