/** @brief Extension (not in the reference): pose-graph optimisation on the device.
 *
 * The consumer of the rest of the API: odometry edges from registerFeatures / a scan sequence, loop edges from a
 * PlaceDatabase match and the registration started from it, each weighted by its RegistrationInformation, corrected
 * together by a sparse SE(3) least-squares solve (Levenberg-Marquardt over block-Jacobi preconditioned conjugate gradients).
 * The rule is written out in loamx.h ("pose graph"); results do not depend on how the device schedules its threads.
 */
#pragma once
#include <array>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "common.h"
#include "geometry.h"
#include "registration.h"

namespace loam {

/// loamx_pgo_params; the defaults are loamx_pgo_default_params'
struct PoseGraphParams {
  uint32_t max_iterations = 20;
  uint32_t max_pcg_iterations = 500;
  double pcg_tolerance = 1e-8;
  double initial_lambda = 1e-4;
  double cost_tolerance = 1e-9;
  double step_tolerance = 1e-10;
  double huber_delta = 0.0;  ///< 0: off
};

/// loamx_pgo_summary
struct PoseGraphSummary {
  enum class TerminationType : uint32_t { COST_CONVERGED = 0, STEP_CONVERGED, MAX_ITERATIONS, LAMBDA_OVERFLOW, NOTHING_TO_DO, BAD_INPUT };
  double initial_cost = 0, final_cost = 0, lambda = 0, max_update = 0;
  size_t iterations = 0, accepted = 0, pcg_iterations = 0;
  TerminationType termination_type = TerminationType::NOTHING_TO_DO;
  size_t n_bad_edges = 0;
};

/// Poses world_T_i and the edges between them; optimize() corrects the poses in place. Pose 0 is fixed unless setFixed says
/// otherwise.
class PoseGraph {
 public:
  explicit PoseGraph(const PoseGraphParams& params = PoseGraphParams()) : params_(params) {}
  PoseGraphParams& params() { return params_; }
  const PoseGraphParams& params() const { return params_; }
  /// Appends a pose; returns its id (ids are consecutive from 0)
  size_t addPose(const Pose3d& world_T_pose) {
    std::array<double, 7> p;
    world_T_pose.toArray(p.data());
    poses_.push_back(p);
    if (any_fixed_) fixed_.push_back(0);
    return poses_.size() - 1;
  }
  /// The first call replaces the default (pose 0 only) by the poses named since
  void setFixed(size_t id, bool fixed = true) {
    if (id >= poses_.size()) throw std::out_of_range("loam::PoseGraph::setFixed: no such pose");
    if (!any_fixed_) fixed_.assign(poses_.size(), 0), any_fixed_ = true;
    fixed_[id] = fixed ? 1 : 0;
  }
  /// a_T_b measures pose b in the frame of pose a; information: row-major 6 x 6 in the basis of RegistrationInformation
  /// (rotation first), only its upper triangle is read
  void addEdge(size_t a, size_t b, const Pose3d& a_T_b, const double information[36]) {
    loamx_pgo_edge e{};
    e.a = static_cast<uint32_t>(a), e.b = static_cast<uint32_t>(b);
    if (a > 0xFFFFFFFFull || b > 0xFFFFFFFFull) throw std::out_of_range("loam::PoseGraph::addEdge: pose id beyond 32 bits");
    a_T_b.toArray(e.a_T_b);
    for (int i = 0; i < 36; i++) e.information[i] = information[i];
    edges_.push_back(e);
  }
  void addEdge(size_t a, size_t b, const Pose3d& a_T_b, const std::vector<double>& information) {
    if (information.size() != 36) throw std::runtime_error("loam::PoseGraph::addEdge: the information matrix holds 6 x 6 entries");
    addEdge(a, b, a_T_b, information.data());
  }
  /// the edge a registration made: target a, source b, its pose and its information matrix
  void addEdge(size_t a, size_t b, const Pose3d& a_T_b, const RegistrationInformation& information) {
    addEdge(a, b, a_T_b, information.information);
  }
  size_t numPoses() const { return poses_.size(); }
  size_t numEdges() const { return edges_.size(); }
  Pose3d pose(size_t id) const { return Pose3d::fromArray(poses_.at(id).data()); }
  bool fixed(size_t id) const { return any_fixed_ ? fixed_.at(id) != 0 : id == 0; }

  /// Solves; the poses are corrected in place. Throws what the C ABI refuses (an invalid edge, no fixed pose, non-finite values).
  PoseGraphSummary optimize() {
    loamx_ctx* ctx = gpu::defaultContext();
    loamx_pgo_params p;
    loamx_pgo_default_params(&p);
    p.max_iterations = params_.max_iterations, p.max_pcg_iterations = params_.max_pcg_iterations, p.pcg_tolerance = params_.pcg_tolerance;
    p.initial_lambda = params_.initial_lambda, p.cost_tolerance = params_.cost_tolerance, p.step_tolerance = params_.step_tolerance;
    p.huber_delta = params_.huber_delta;
    loamx_pgo_summary s{};
    gpu::check(ctx, loamx_pose_graph_optimize(ctx, poses_.empty() ? nullptr : poses_.front().data(), poses_.size(),
                                              any_fixed_ ? fixed_.data() : nullptr, edges_.data(), edges_.size(), &p, &s));
    PoseGraphSummary out;
    out.initial_cost = s.initial_cost, out.final_cost = s.final_cost, out.lambda = s.lambda, out.max_update = s.max_update;
    out.iterations = s.iterations, out.accepted = s.accepted, out.pcg_iterations = s.pcg_iterations;
    out.termination_type = static_cast<PoseGraphSummary::TerminationType>(s.termination);
    out.n_bad_edges = s.n_bad_edges;
    return out;
  }

 private:
  PoseGraphParams params_;
  std::vector<std::array<double, 7>> poses_;
  std::vector<uint8_t> fixed_;
  bool any_fixed_ = false;
  std::vector<loamx_pgo_edge> edges_;
};

}  // namespace loam
