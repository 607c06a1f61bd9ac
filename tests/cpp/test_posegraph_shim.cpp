// test_posegraph_shim.cpp — loam::PoseGraph (include/loam/posegraph.h) through the C++ headers: on a 12-pose ring with one loop
// the corrected poses and the summary are the C ABI's (loamx_pose_graph_optimize on the same arrays) byte for byte, the defaults
// are loamx_pgo_default_params', and what the C ABI refuses is thrown.
// Built and run by tests/test_gpu_posegraph_modules.py (needs a GPU).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "loam/loam.h"

using namespace loam;

static int g_failures = 0, g_checks = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    g_checks++;                                                            \
    if (!(cond)) {                                                         \
      g_failures++;                                                        \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
    }                                                                      \
  } while (0)

static Pose3d ring_pose(int i, int n) {
  const double th = 6.283185307179586 * i / n;
  return Pose3d(Quaterniond(std::cos(th / 2 + 0.4), 0.0, 0.0, std::sin(th / 2 + 0.4)), Vector3d(8.0 * std::cos(th), 8.0 * std::sin(th), 0.05 * i));
}

int main() {
  PoseGraphParams params;
  loamx_pgo_params cp;
  loamx_pgo_default_params(&cp);
  CHECK(cp.max_iterations == params.max_iterations && cp.max_pcg_iterations == params.max_pcg_iterations && cp.pcg_tolerance == params.pcg_tolerance &&
        cp.initial_lambda == params.initial_lambda && cp.cost_tolerance == params.cost_tolerance && cp.step_tolerance == params.step_tolerance &&
        cp.huber_delta == params.huber_delta);
  CHECK(params.max_iterations == 20 && params.max_pcg_iterations == 500 && params.pcg_tolerance == 1e-8 && params.initial_lambda == 1e-4 &&
        params.cost_tolerance == 1e-9 && params.step_tolerance == 1e-10 && params.huber_delta == 0.0);

  // the ring: measurements from the truth, a start that has drifted off it
  const int n = 12;
  PoseGraph graph(params);
  std::vector<double> poses(7 * n);
  std::vector<loamx_pgo_edge> edges;
  double info[36] = {0};
  for (int k = 0; k < 6; k++) info[7 * k] = k < 3 ? 900.0 : 100.0;
  info[1] = 30.0, info[6] = -777.0;  // (the lower triangle is never read)
  for (int i = 0; i < n; i++) {
    Pose3d p = ring_pose(i, n);
    p.translation = p.translation + Vector3d(0.02 * i, -0.015 * i, 0.01 * i);
    CHECK(graph.addPose(p) == (size_t)i);
    p.toArray(&poses[7 * i]);
  }
  for (int i = 0; i < n; i++) {
    const int a = i, b = (i + 1) % n;
    const Pose3d z = ring_pose(a, n).inverse().compose(ring_pose(b, n));
    graph.addEdge(a, b, z, info);
    loamx_pgo_edge e{};
    e.a = a, e.b = b;
    z.toArray(e.a_T_b);
    std::memcpy(e.information, info, sizeof(info));
    edges.push_back(e);
  }
  CHECK(graph.numPoses() == 12 && graph.numEdges() == 12 && graph.fixed(0) && !graph.fixed(1));

  loamx_ctx* ctx = gpu::defaultContext();
  loamx_pgo_summary cs{};
  CHECK(loamx_pose_graph_optimize(ctx, poses.data(), n, nullptr, edges.data(), edges.size(), &cp, &cs) == LOAMX_OK);
  const PoseGraphSummary s = graph.optimize();
  CHECK(s.initial_cost == cs.initial_cost && s.final_cost == cs.final_cost && s.lambda == cs.lambda && s.max_update == cs.max_update);
  CHECK(s.iterations == cs.iterations && s.accepted == cs.accepted && s.pcg_iterations == cs.pcg_iterations && s.n_bad_edges == 0);
  CHECK((uint32_t)s.termination_type == cs.termination);
  // (the measurements are exact: the solve ends on a vanishing cost or on a vanishing step)
  CHECK(s.termination_type == PoseGraphSummary::TerminationType::COST_CONVERGED || s.termination_type == PoseGraphSummary::TerminationType::STEP_CONVERGED);
  CHECK(s.final_cost < 1e-3 * s.initial_cost && s.accepted >= 1);
  for (int i = 0; i < n; i++) {
    double got[7];
    graph.pose(i).toArray(got);
    CHECK(std::memcmp(got, &poses[7 * i], sizeof(got)) == 0);
    CHECK((graph.pose(i).translation - ring_pose(i, n).translation).norm() < 0.1);
  }

  // fixed poses: the first setFixed replaces the default
  graph.setFixed(5);
  CHECK(!graph.fixed(0) && graph.fixed(5));
  graph.setFixed(5, false);
  bool threw = false;
  try {
    graph.optimize();  // no pose is fixed
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);
  graph.setFixed(0);
  // an edge to a pose that does not exist is refused, and the graph goes on working without it
  PoseGraph bad(params);
  bad.addPose(Pose3d::Identity()), bad.addPose(Pose3d::Identity());
  bad.addEdge(0, 7, Pose3d::Identity(), info);
  threw = false;
  try {
    bad.optimize();
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);
  RegistrationInformation ri{};
  for (int k = 0; k < 6; k++) ri.information[7 * k] = 50.0;
  PoseGraph two(params);
  two.addPose(Pose3d::Identity()), two.addPose(Pose3d(Quaterniond::Identity(), Vector3d(1.0, 0.0, 0.0)));
  two.addEdge(0, 1, Pose3d(Quaterniond::Identity(), Vector3d(2.0, 0.0, 0.0)), ri);
  const PoseGraphSummary s2 = two.optimize();
  CHECK(s2.accepted >= 1 && std::fabs(two.pose(1).translation(0) - 2.0) < 1e-9);
  CHECK(PoseGraph().optimize().termination_type == PoseGraphSummary::TerminationType::NOTHING_TO_DO);

  std::printf("posegraph shim: %d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
