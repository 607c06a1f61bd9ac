/** @brief Extension (not in the reference): the surfel map on the device, per voxel the mean, the covariance and the normal.
 *
 * A SurfelMap takes scans (or any clouds) at their poses like a CloudMap and keeps, per voxel, integer first and second moments
 * and a sum of the directions back to the sensor. It reads out one Surfel per voxel in order of first appearance: mean,
 * covariance, eigenvalues ascending, and the unit normal turned towards where the voxel was seen from; query() looks up the
 * surfel of a point and its signed distance to the surfel's plane. The sums are integers, so the map does not depend on how the
 * device schedules its threads. The rule is written out in loamx.h ("surfel map").
 *
 * localize() places a cloud in the map: point-to-plane Gauss-Newton against the voxels' fitted planes, solved on the device
 * (loamx.h, "surfel localisation").
 */
#pragma once
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <vector>

#include "common.h"
#include "geometry.h"
#include "registration.h"

namespace loam {

/// loamx_surfel_map_params; the defaults are loamx_default_surfel_map_params'
struct SurfelMapParams {
  double leaf = 0.5;         ///< voxel edge
  double min_range = 0.5;    ///< points nearer to the sensor are dropped (the all-zero cells of an organised scan among them)
  double max_range = 120.0;  ///< points farther from the sensor are dropped
};

/// loamx_surfel_map_stats
struct SurfelMapStats {
  uint64_t voxels = 0, points_offered = 0, points_used = 0, invalid = 0, range = 0, outside = 0, overflow = 0;
};

/// One voxel: loamx_surfel, field for field (128 bytes)
using Surfel = loamx_surfel;
static_assert(sizeof(Surfel) == 128, "loamx_surfel is 128 bytes");

/// What SurfelMap::query returns, entry i for point i: the surfel of its voxel (zero bytes without one), the signed distance
/// normal . (p - mean) and the voxel's count (0 without one)
struct SurfelQuery {
  std::vector<Surfel> surfels;
  std::vector<double> distances;
  std::vector<uint32_t> counts;
  size_t size() const { return counts.size(); }
};

/// loamx_localize_params; the defaults are loamx_default_localize_params'
struct LocalizeParams {
  uint32_t neighborhood = 7;      ///< 7: the home voxel and its six face neighbours; 1: the home voxel only
  uint32_t min_points = 5;        ///< a voxel with fewer points offers no plane
  double planarity = 0.1;         ///< a plane needs eval[0] <= planarity eval[1]
  double max_distance = 0.0;      ///< gate on the point-to-plane distance; 0: the map's leaf
  double huber_delta = 0.1;       ///< 0: no Huber
  uint32_t max_iterations = 10;
  uint32_t min_rows = 100;
  double rotation_convergence_thresh = 1e-3;
  double position_convergence_thresh = 1e-2;
  double min_eigenvalue_per_row = 1e-3;  ///< a direction is solved for where its eigenvalue exceeds this times the rows
};

/// loamx_localize_result, field for field (128 bytes); termination: LOAMX_LOCALIZE_*
using LocalizeResult = loamx_localize_result;
static_assert(sizeof(LocalizeResult) == 128, "loamx_localize_result is 128 bytes");

/// What SurfelMap::localize returns: the pose, the record of the solve and the information matrix at the pose
struct Localization {
  Pose3d map_T_cloud;
  LocalizeResult result;
  RegistrationInformation information;
  bool converged() const { return result.termination == LOAMX_LOCALIZE_CONVERGED; }
};

/// The map (loamx_surfel_map): table, voxel list and counters on the device. Cheap to copy (shared handle).
class SurfelMap {
 public:
  explicit SurfelMap(const SurfelMapParams& params = SurfelMapParams(), size_t max_voxels = (size_t)1 << 20) : params_(params), max_voxels_(max_voxels) {
    loamx_ctx* ctx = gpu::defaultContext();
    loamx_surfel_map_params p;
    loamx_default_surfel_map_params(&p);
    p.leaf = params.leaf, p.min_range = params.min_range, p.max_range = params.max_range;
    loamx_surfel_map* h = nullptr;
    gpu::check(ctx, loamx_surfel_map_create(ctx, &p, max_voxels, &h));
    handle_ = std::shared_ptr<loamx_surfel_map>(h, [](loamx_surfel_map* m) { loamx_surfel_map_destroy(gpu::defaultContext(), m); });
  }
  const SurfelMapParams& params() const { return params_; }
  size_t maxVoxels() const { return max_voxels_; }
  /// One cloud in the sensor frame at world_T_sensor: the normals of its voxels turn towards the pose's translation. Float fields
  /// read through FieldAccessor travel as floats, like the scans of extractFeatures.
  template <template <typename> class Accessor = FieldAccessor, typename PointType, typename Alloc>
  void add(const std::vector<PointType, Alloc>& points, const Pose3d& world_T_sensor) {
    double pose[7];
    world_T_sensor.toArray(pose);
    addPacked<Accessor>(points, pose);
  }
  /// One cloud that is in the map frame already (no transform; seen from the origin)
  template <template <typename> class Accessor = FieldAccessor, typename PointType, typename Alloc>
  void add(const std::vector<PointType, Alloc>& points) {
    addPacked<Accessor>(points, nullptr);
  }
  void clear() {
    loamx_ctx* ctx = gpu::defaultContext();
    gpu::check(ctx, loamx_surfel_map_clear(ctx, handle_.get()));
  }
  /// Removes the voxels outside the box center + [lo, hi] (metres, map frame, widened to voxel boundaries; loamx.h, "map window"):
  /// the map keeps following the sensor at a fixed max_voxels. Infinite bounds are allowed. Synchronises.
  MapCrop crop(const std::array<double, 3>& lo, const std::array<double, 3>& hi, const std::array<double, 3>& center = {0.0, 0.0, 0.0}) {
    return gpu::cropWindow(loamx_surfel_map_crop, handle_.get(), lo, hi, center);
  }
  /// The voxels that hold at least min_points points, in order of first appearance
  std::vector<Surfel> surfels(uint32_t min_points = 1) const {
    loamx_ctx* ctx = gpu::defaultContext();
    const size_t room = (size_t)stats().voxels;
    std::vector<Surfel> out(room);
    size_t n = 0;
    gpu::check(ctx, loamx_surfel_map_emit_host(ctx, handle_.get(), min_points, out.data(), room, &n));
    out.resize(n < room ? n : room);
    return out;
  }
  /// The surfels of the voxels of n points (xyz: 3 n doubles, map frame) that hold at least min_points points
  SurfelQuery query(const std::vector<double>& xyz, uint32_t min_points = 1) const {
    if (xyz.size() % 3) throw std::runtime_error("SurfelMap::query: xyz holds 3 doubles per point");
    loamx_ctx* ctx = gpu::defaultContext();
    const size_t n = xyz.size() / 3;
    SurfelQuery out;
    out.surfels.resize(n), out.distances.resize(n), out.counts.resize(n);
    if (n == 0) return out;
    const size_t o_rec = 24 * n, o_dist = o_rec + sizeof(Surfel) * n, o_cnt = o_dist + 8 * n;  // (all multiples of 8)
    void* block = nullptr;
    gpu::check(ctx, loamx_dev_alloc(ctx, o_cnt + 4 * n, &block));
    std::shared_ptr<void> guard(block, [ctx](void* p) { loamx_dev_free(ctx, p); });
    char* b = static_cast<char*>(block);
    gpu::check(ctx, loamx_copy_to_device(ctx, b, xyz.data(), 24 * n));
    gpu::check(ctx, loamx_surfel_map_query(ctx, handle_.get(), reinterpret_cast<const double*>(b), 3, n, min_points,
                                           reinterpret_cast<loamx_surfel*>(b + o_rec), reinterpret_cast<double*>(b + o_dist),
                                           reinterpret_cast<uint32_t*>(b + o_cnt)));
    gpu::check(ctx, loamx_copy_to_host(ctx, out.surfels.data(), b + o_rec, sizeof(Surfel) * n));
    gpu::check(ctx, loamx_copy_to_host(ctx, out.distances.data(), b + o_dist, 8 * n));
    gpu::check(ctx, loamx_copy_to_host(ctx, out.counts.data(), b + o_cnt, 4 * n));
    return out;
  }
  SurfelMapStats stats() const {
    loamx_ctx* ctx = gpu::defaultContext();
    loamx_surfel_map_stats s;
    gpu::check(ctx, loamx_surfel_map_stats_read(ctx, handle_.get(), &s));
    SurfelMapStats out;
    out.voxels = s.voxels, out.points_offered = s.points_offered, out.points_used = s.points_used, out.invalid = s.invalid;
    out.range = s.range, out.outside = s.outside, out.overflow = s.overflow;
    return out;
  }
  /// Places one cloud (sensor frame) in the map, starting from `init` = map_T_cloud. The map is not changed. The localiser behind
  /// it is kept between calls and made anew when a larger cloud arrives.
  template <template <typename> class Accessor = FieldAccessor, typename PointType, typename Alloc>
  Localization localize(const std::vector<PointType, Alloc>& points, const Pose3d& init, const LocalizeParams& params = LocalizeParams()) {
    loamx_ctx* ctx = gpu::defaultContext();
    loamx_localize_params p;
    loamx_default_localize_params(&p);
    p.neighborhood = params.neighborhood, p.min_points = params.min_points, p.planarity = params.planarity;
    p.max_distance = params.max_distance, p.huber_delta = params.huber_delta, p.max_iterations = params.max_iterations;
    p.min_rows = params.min_rows, p.rotation_convergence_thresh = params.rotation_convergence_thresh;
    p.position_convergence_thresh = params.position_convergence_thresh, p.min_eigenvalue_per_row = params.min_eigenvalue_per_row;
    double pose[7];
    init.toArray(pose);
    loamx_surfel_localizer* loc = localizer(points.size());
    Localization out;
    loamx_reg_information info;
    if constexpr (gpu::float_scan_v<Accessor, PointType>) {
      const std::vector<float> xyz = gpu::packFloat(points);
      gpu::check(ctx, loamx_surfel_localizer_run_host_f32(ctx, loc, xyz.data(), 3, points.size(), pose, &p, &out.result, &info));
    } else {
      const std::vector<double> xyz = gpu::pack<Accessor>(points);
      gpu::check(ctx, loamx_surfel_localizer_run_host(ctx, loc, xyz.data(), 3, points.size(), pose, &p, &out.result, &info));
    }
    out.map_T_cloud = Pose3d::fromArray(out.result.pose);
    out.information = gpu::fromC(info);
    return out;
  }
  loamx_surfel_map* handle() const { return handle_.get(); }
  /// the localiser for clouds of up to n_points points (kept; destroyed before the map it reads)
  loamx_surfel_localizer* localizer(size_t n_points) {
    if (!localizer_ || localizer_points_ < n_points) {
      loamx_ctx* ctx = gpu::defaultContext();
      localizer_.reset();
      loamx_surfel_localizer* h = nullptr;
      const size_t room = n_points > 4096 ? n_points : 4096;
      gpu::check(ctx, loamx_surfel_localizer_create(ctx, handle_.get(), 1, room, &h));
      std::shared_ptr<loamx_surfel_map> keep = handle_;  // (the map outlives its localiser)
      localizer_ = std::shared_ptr<loamx_surfel_localizer>(h, [keep](loamx_surfel_localizer* l) { loamx_surfel_localizer_destroy(gpu::defaultContext(), l); });
      localizer_points_ = room;
    }
    return localizer_.get();
  }

 private:
  template <template <typename> class Accessor, typename PointType, typename Alloc>
  void addPacked(const std::vector<PointType, Alloc>& points, const double* pose) {
    loamx_ctx* ctx = gpu::defaultContext();
    if constexpr (gpu::float_scan_v<Accessor, PointType>) {
      const std::vector<float> xyz = gpu::packFloat(points);
      gpu::check(ctx, loamx_surfel_map_add_cloud_host_f32(ctx, handle_.get(), xyz.data(), 3, points.size(), pose));
    } else {
      const std::vector<double> xyz = gpu::pack<Accessor>(points);
      gpu::check(ctx, loamx_surfel_map_add_cloud_host(ctx, handle_.get(), xyz.data(), 3, points.size(), pose));
    }
  }

  SurfelMapParams params_;
  size_t max_voxels_;
  std::shared_ptr<loamx_surfel_map> handle_;
  std::shared_ptr<loamx_surfel_localizer> localizer_;
  size_t localizer_points_ = 0;
};

}  // namespace loam
