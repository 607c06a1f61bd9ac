/** @brief LOAM feature registration — drop-in for the reference's loam/include/loam/registration.h.
 * Same template, parameter / detail structs and defaults; the iterative closest feature loop
 * (association, line / plane fits, robust Levenberg-Marquardt) runs on the MI355X through
 * loamx_register_features.
 */
#pragma once
#include <memory>
#include <stdexcept>
#include <utility>
#include <vector>

#include "common.h"
#include "features.h"
#include "geometry.h"
#include "kdtree.h"

namespace loam {

/// Registration parameters (reference registration.h:40-75; same field order and defaults)
struct RegistrationParams {
  size_t num_edge_neighbors{5};
  double max_edge_neighbor_dist{1.0};
  size_t min_line_fit_points{3};
  double min_line_condition_number{10};
  size_t num_plane_neighbors{5};
  double max_plane_neighbor_dist{2.0};
  size_t min_plane_fit_points{4};
  double max_avg_point_plane_dist{0.1};
  size_t max_iterations{10};
  double rotation_convergence_thresh{1e-3};
  double position_convergence_thresh{1e-2};
  size_t min_associations{100};
};

/// Detailed information about one registration (reference registration.h:79-109)
struct RegistrationDetail {
  enum TerminationType { CONVERGED, MAX_ITER, INSUFFICIENT_ASSOCIATIONS };
  struct IterationInfo {
    Pose3d target_T_source_init;
    std::vector<std::pair<size_t, size_t>> edge_associations;
    std::vector<std::pair<size_t, size_t>> plane_associations;
    Pose3d estimate_update;
    IterationInfo(const Pose3d target_T_source_init, const std::vector<std::pair<size_t, size_t>> edge_associations,
                  const std::vector<std::pair<size_t, size_t>> plane_associations, const Pose3d estimate_update)
        : target_T_source_init(target_T_source_init),
          edge_associations(edge_associations),
          plane_associations(plane_associations),
          estimate_update(estimate_update) {}
  };
  std::vector<IterationInfo> iteration_info;
  TerminationType termination_type;
};

namespace gpu {
inline loamx_reg_params toC(const RegistrationParams& p) {
  return loamx_reg_params{p.num_edge_neighbors,     p.max_edge_neighbor_dist,      p.min_line_fit_points,
                          p.min_line_condition_number, p.num_plane_neighbors,      p.max_plane_neighbor_dist,
                          p.min_plane_fit_points,   p.max_avg_point_plane_dist,    p.max_iterations,
                          p.rotation_convergence_thresh, p.position_convergence_thresh, p.min_associations};
}
/// The buffers behind a loamx_reg_detail for one registration, and their way back into a RegistrationDetail
/// (nothing is allocated or captured when `detail` is null).
class DetailCapture {
 public:
  DetailCapture(std::shared_ptr<RegistrationDetail> detail, size_t n_se, size_t n_sp, size_t mi) : detail_(std::move(detail)) {
    if (!detail_) return;
    info_.resize(mi ? mi : 1);
    edge_pairs_.resize(2 * (n_se ? n_se : 1) * (mi ? mi : 1));
    plane_pairs_.resize(2 * (n_sp ? n_sp : 1) * (mi ? mi : 1));
    n_edge_pairs_.assign(mi ? mi : 1, 0);
    n_plane_pairs_.assign(mi ? mi : 1, 0);
    c_.iter_info = info_.data();
    c_.edge_pairs = edge_pairs_.data(), c_.pairs_cap_edge = n_se ? n_se : 1, c_.n_edge_pairs = n_edge_pairs_.data();
    c_.plane_pairs = plane_pairs_.data(), c_.pairs_cap_plane = n_sp ? n_sp : 1, c_.n_plane_pairs = n_plane_pairs_.data();
  }
  loamx_reg_detail* arg() { return detail_ ? &c_ : nullptr; }
  void finish(const loamx_reg_result& result) {
    if (!detail_) return;
    for (uint32_t it = 0; it < c_.n_iter_info; it++) {
      std::vector<std::pair<size_t, size_t>> ea, pa;
      const uint32_t* e = edge_pairs_.data() + (size_t)it * 2 * c_.pairs_cap_edge;
      const uint32_t* p = plane_pairs_.data() + (size_t)it * 2 * c_.pairs_cap_plane;
      for (uint32_t k = 0; k < n_edge_pairs_[it]; k++) ea.emplace_back(e[2 * k], e[2 * k + 1]);
      for (uint32_t k = 0; k < n_plane_pairs_[it]; k++) pa.emplace_back(p[2 * k], p[2 * k + 1]);
      detail_->iteration_info.emplace_back(Pose3d::fromArray(info_[it].target_T_source_init), ea, pa,
                                           Pose3d::fromArray(info_[it].estimate_update));
    }
    detail_->termination_type = static_cast<RegistrationDetail::TerminationType>(result.termination);
  }

 private:
  std::shared_ptr<RegistrationDetail> detail_;
  std::vector<loamx_iter_info> info_;
  std::vector<uint32_t> edge_pairs_, plane_pairs_, n_edge_pairs_, n_plane_pairs_;
  loamx_reg_detail c_{};
};
}  // namespace gpu

/// Registers source to target, returning target_T_source (reference registration.h:128-131)
template <template <typename> class Accessor = FieldAccessor, typename PointType, template <typename> class Alloc>
Pose3d registerFeatures(const LoamFeatures<PointType, Alloc>& source, const LoamFeatures<PointType, Alloc>& target,
                        const Pose3d& target_T_source_init, const RegistrationParams& params = RegistrationParams(),
                        std::shared_ptr<RegistrationDetail> detail = nullptr) {
  loamx_ctx* ctx = gpu::defaultContext();
  const std::vector<double> se = gpu::pack<Accessor>(source.edge_points), sp = gpu::pack<Accessor>(source.planar_points);
  const std::vector<double> te = gpu::pack<Accessor>(target.edge_points), tp = gpu::pack<Accessor>(target.planar_points);
  const loamx_reg_params rp = gpu::toC(params);
  double init[7];
  target_T_source_init.toArray(init);
  loamx_reg_result result{};
  gpu::DetailCapture capture(detail, source.edge_points.size(), source.planar_points.size(), params.max_iterations);
  gpu::check(ctx, loamx_register_features(ctx, se.data(), source.edge_points.size(), sp.data(), source.planar_points.size(), te.data(),
                                          target.edge_points.size(), tp.data(), target.planar_points.size(), init, &rp, &result,
                                          capture.arg()));
  capture.finish(result);
  return Pose3d::fromArray(result.pose);
}


/** @brief Extension (not in the reference): the spatial index of a target feature set built once and
 * kept on the device, for scan-to-map registration against a slowly changing local map. The
 * reference rebuilds both KD-trees on every call (registration-inl.h:20-23). The map is kept up on the device as
 * well: insert / insertFiltered add a registered scan's features, crop drops what has left the local window,
 * edgePoints / planarPoints read it back. */
class TargetIndex {
 public:
  template <template <typename> class Accessor = FieldAccessor, typename PointType, template <typename> class Alloc>
  static TargetIndex build(const LoamFeatures<PointType, Alloc>& target, const RegistrationParams& params = RegistrationParams()) {
    loamx_ctx* ctx = gpu::defaultContext();
    const std::vector<double> te = gpu::pack<Accessor>(target.edge_points), tp = gpu::pack<Accessor>(target.planar_points);
    const loamx_reg_params rp = gpu::toC(params);
    loamx_target_index* h = nullptr;
    gpu::check(ctx, loamx_target_index_create(ctx, te.data(), target.edge_points.size(), tp.data(),
                                              target.planar_points.size(), &rp, &h));
    return TargetIndex(h);
  }
  /// Appends features to the target (a map that grows scan by scan): afterwards the index is the one `build`
  /// gives for the concatenated feature sets.
  template <template <typename> class Accessor = FieldAccessor, typename PointType, template <typename> class Alloc>
  void insert(const LoamFeatures<PointType, Alloc>& more) {
    const std::vector<double> e = gpu::pack<Accessor>(more.edge_points), p = gpu::pack<Accessor>(more.planar_points);
    gpu::check(gpu::defaultContext(), loamx_target_index_insert(gpu::defaultContext(), handle_.get(), e.data(), more.edge_points.size(),
                                                                p.data(), more.planar_points.size()));
  }
  /// Map upkeep after a registration (loamx.h, "map upkeep"): moves the scan's features into the map frame with
  /// world_T_scan (the arithmetic of Pose3d::act), thins them on a voxel grid — a point is added unless its voxel (edge
  /// length edge_leaf / planar_leaf; <= 0: no filter for that kind) already holds a point of the map or an earlier point
  /// of this call — and appends the rest as `insert` would. Returns the points added {edge, planar}.
  template <template <typename> class Accessor = FieldAccessor, typename PointType, template <typename> class Alloc>
  std::pair<size_t, size_t> insertFiltered(const LoamFeatures<PointType, Alloc>& more, const Pose3d& world_T_scan, double edge_leaf,
                                           double planar_leaf) {
    const std::vector<double> e = gpu::pack<Accessor>(more.edge_points), p = gpu::pack<Accessor>(more.planar_points);
    double pose[7];
    world_T_scan.toArray(pose);
    size_t ne = 0, np = 0;
    gpu::check(gpu::defaultContext(),
               loamx_target_index_insert_filtered(gpu::defaultContext(), handle_.get(), e.data(), more.edge_points.size(), p.data(),
                                                  more.planar_points.size(), pose, edge_leaf, planar_leaf, &ne, &np));
    return {ne, np};
  }
  /// Keeps the points with lo <= p <= hi on every axis (the local window around the vehicle); the index afterwards is the
  /// one `build` gives for the survivors in their order. Returns the points removed {edge, planar}.
  std::pair<size_t, size_t> crop(const Vector3d& lo, const Vector3d& hi) {
    const double l[3] = {lo(0), lo(1), lo(2)}, h[3] = {hi(0), hi(1), hi(2)};
    size_t ne = 0, np = 0;
    gpu::check(gpu::defaultContext(), loamx_target_index_crop(gpu::defaultContext(), handle_.get(), l, h, &ne, &np));
    return {ne, np};
  }
  /// The map's points in index order (read back from the device); the *Rows forms return them packed row-major (n x 3).
  std::vector<double> edgePointRows() const { return pointRows(0); }
  std::vector<double> planarPointRows() const { return pointRows(1); }
  std::vector<Vector3d> edgePoints() const { return unpack(pointRows(0)); }
  std::vector<Vector3d> planarPoints() const { return unpack(pointRows(1)); }
  size_t numEdgePoints() const {
    size_t n = 0;
    loamx_target_index_size(handle_.get(), &n, nullptr);
    return n;
  }
  size_t numPlanarPoints() const {
    size_t n = 0;
    loamx_target_index_size(handle_.get(), nullptr, &n);
    return n;
  }
  const loamx_target_index* handle() const { return handle_.get(); }

 private:
  explicit TargetIndex(loamx_target_index* h)
      : handle_(h, [](loamx_target_index* p) { loamx_target_index_destroy(gpu::defaultContext(), p); }) {}
  std::vector<double> pointRows(int which_set) const {
    const size_t n = which_set ? numPlanarPoints() : numEdgePoints();
    std::vector<double> xyz(3 * n);
    gpu::check(gpu::defaultContext(), loamx_target_index_points(gpu::defaultContext(), handle_.get(), which_set, 0, n, xyz.data()));
    return xyz;
  }
  static std::vector<Vector3d> unpack(const std::vector<double>& xyz) {
    std::vector<Vector3d> out;
    out.reserve(xyz.size() / 3);
    for (size_t i = 0; i + 2 < xyz.size(); i += 3) out.emplace_back(xyz[i], xyz[i + 1], xyz[i + 2]);
    return out;
  }
  std::shared_ptr<loamx_target_index> handle_;
};

/// registerFeatures against a prebuilt TargetIndex (params must carry the neighbour radii the index was built with)
template <template <typename> class Accessor = FieldAccessor, typename PointType, template <typename> class Alloc>
Pose3d registerFeatures(const LoamFeatures<PointType, Alloc>& source, const TargetIndex& target,
                        const Pose3d& target_T_source_init, const RegistrationParams& params = RegistrationParams(),
                        std::shared_ptr<RegistrationDetail> detail = nullptr) {
  loamx_ctx* ctx = gpu::defaultContext();
  const std::vector<double> se = gpu::pack<Accessor>(source.edge_points), sp = gpu::pack<Accessor>(source.planar_points);
  const loamx_reg_params rp = gpu::toC(params);
  double init[7];
  target_T_source_init.toArray(init);
  loamx_reg_result result{};
  gpu::DetailCapture capture(detail, source.edge_points.size(), source.planar_points.size(), params.max_iterations);
  gpu::check(ctx, loamx_register_features_indexed(ctx, target.handle(), se.data(), source.edge_points.size(), sp.data(),
                                                  source.planar_points.size(), init, &rp, &result, capture.arg()));
  capture.finish(result);
  return Pose3d::fromArray(result.pose);
}

/** @brief Extension (not in the reference): the 6x6 Gauss-Newton information matrix H = sum J^T J of the registration residuals of a
 * pair at a pose, with its eigen-decomposition (loamx.h: loamx_reg_information). Basis: the left perturbation
 * target_T_source <- Exp([omega, t]) o target_T_source — omega a rotation vector in radians about the target frame's axes
 * (entries 0-2), t in metres (entries 3-5), rotation first. What a pose graph or a filter needs next to the pose, and what
 * LOAM's mapping thread thresholds to detect corridors, tunnels and open fields. */
struct RegistrationInformation {
  double information[36];   ///< H, row-major, symmetric
  double eigenvalues[6];    ///< ascending
  double eigenvectors[36];  ///< row i: unit eigenvector of eigenvalues[i]
  double gradient[6];       ///< sum J^T r: near zero where the pose sits at a minimum
  double weighted_sq_error; ///< sum of the (Huber-scaled) squared residuals
  size_t n_edge, n_plane;   ///< rows that entered the sums
  size_t n_huber;           ///< of those, rows beyond the Huber threshold
  size_t n_dropped;         ///< valid associations left out (non-finite row)

  /// sigma^2 * sum v_i v_i^T / lambda_i over lambda_i > rel_threshold * lambda_5 with sigma^2 = weighted_sq_error / (rows - 6):
  /// the covariance of the pose in the observable directions, row-major 6x6. Throws where there are not more than 6 rows.
  std::vector<double> covariance(double rel_threshold = 1e-12) const {
    const size_t rows = n_edge + n_plane;
    if (rows <= 6) throw std::runtime_error("RegistrationInformation::covariance: not more than 6 residual rows");
    const double sigma2 = weighted_sq_error / static_cast<double>(rows - 6);
    std::vector<double> cov(36, 0.0);
    for (int i = 0; i < 6; i++) {
      if (!(eigenvalues[i] > rel_threshold * eigenvalues[5])) continue;
      for (int a = 0; a < 6; a++)
        for (int b = 0; b < 6; b++) cov[6 * a + b] += eigenvectors[6 * i + a] * eigenvectors[6 * i + b] / eigenvalues[i];
    }
    for (double& c : cov) c *= sigma2;
    return cov;
  }
  /// The eigenvectors (6 entries each) whose eigenvalue lies below min_eigenvalue: the directions the geometry leaves open.
  std::vector<std::vector<double>> degenerateDirections(double min_eigenvalue) const {
    std::vector<std::vector<double>> out;
    for (int i = 0; i < 6; i++)
      if (eigenvalues[i] < min_eigenvalue) out.emplace_back(eigenvectors + 6 * i, eigenvectors + 6 * i + 6);
    return out;
  }
};

namespace gpu {
inline RegistrationInformation fromC(const loamx_reg_information& c) {
  RegistrationInformation r{};
  for (int i = 0; i < 36; i++) r.information[i] = c.information[i], r.eigenvectors[i] = c.eigenvectors[i];
  for (int i = 0; i < 6; i++) r.eigenvalues[i] = c.eigenvalues[i], r.gradient[i] = c.gradient[i];
  r.weighted_sq_error = c.weighted_sq_error;
  r.n_edge = c.n_edge, r.n_plane = c.n_plane, r.n_huber = c.n_huber, r.n_dropped = c.n_dropped;
  return r;
}
}  // namespace gpu

/// The information matrix of the residuals of (source, target) at target_T_source: one association pass, no solve.
template <template <typename> class Accessor = FieldAccessor, typename PointType, template <typename> class Alloc>
RegistrationInformation registrationInformation(const LoamFeatures<PointType, Alloc>& source, const LoamFeatures<PointType, Alloc>& target,
                                                const Pose3d& target_T_source, const RegistrationParams& params = RegistrationParams()) {
  loamx_ctx* ctx = gpu::defaultContext();
  const std::vector<double> se = gpu::pack<Accessor>(source.edge_points), sp = gpu::pack<Accessor>(source.planar_points);
  const std::vector<double> te = gpu::pack<Accessor>(target.edge_points), tp = gpu::pack<Accessor>(target.planar_points);
  const loamx_reg_params rp = gpu::toC(params);
  double pose[7];
  target_T_source.toArray(pose);
  loamx_reg_information info{};
  gpu::check(ctx, loamx_registration_information(ctx, se.data(), source.edge_points.size(), sp.data(), source.planar_points.size(), te.data(),
                                                 target.edge_points.size(), tp.data(), target.planar_points.size(), pose, &rp, &info));
  return gpu::fromC(info);
}

/// ... against a prebuilt TargetIndex (scan-to-map: where degeneracy matters most)
template <template <typename> class Accessor = FieldAccessor, typename PointType, template <typename> class Alloc>
RegistrationInformation registrationInformation(const LoamFeatures<PointType, Alloc>& source, const TargetIndex& target,
                                                const Pose3d& target_T_source, const RegistrationParams& params = RegistrationParams()) {
  loamx_ctx* ctx = gpu::defaultContext();
  const std::vector<double> se = gpu::pack<Accessor>(source.edge_points), sp = gpu::pack<Accessor>(source.planar_points);
  const loamx_reg_params rp = gpu::toC(params);
  double pose[7];
  target_T_source.toArray(pose);
  loamx_reg_information info{};
  gpu::check(ctx, loamx_registration_information_indexed(ctx, target.handle(), se.data(), source.edge_points.size(), sp.data(),
                                                         source.planar_points.size(), pose, &rp, &info));
  return gpu::fromC(info);
}

}  // namespace loam
