/** @brief Extension (not in the reference): the global map on the device, a centroid voxel grid of posed clouds.
 *
 * A CloudMap takes scans (or any clouds) at their poses and keeps one centroid per voxel: what PCL's VoxelGrid makes of the
 * assembled cloud. The sums are integers, so the map does not depend on how the device schedules its threads, and the voxels
 * come out in order of first appearance. After a pose-graph correction: clear() and add the scans again at the corrected poses.
 * The rule is written out in loamx.h ("cloud map").
 */
#pragma once
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <vector>

#include "common.h"
#include "geometry.h"

namespace loam {

/// loamx_cloud_map_params; the defaults are loamx_default_cloud_map_params'
struct CloudMapParams {
  double leaf = 0.2;         ///< voxel edge
  double min_range = 0.5;    ///< points nearer to the sensor are dropped (the all-zero cells of an organised scan among them)
  double max_range = 120.0;  ///< points farther from the sensor are dropped
};

/// loamx_cloud_map_stats
struct CloudMapStats {
  uint64_t voxels = 0, points_offered = 0, points_used = 0, invalid = 0, range = 0, outside = 0, overflow = 0;
};

/// What CloudMap::points returns: xyz[3 i ..] is the centroid of voxel i of the list, counts[i] its points, first[i] the
/// running index of the point that opened it
struct CloudMapPoints {
  std::vector<double> xyz;
  std::vector<uint32_t> counts, first;
  size_t size() const { return counts.size(); }
};

/// The map (loamx_cloud_map): table, voxel list and counters on the device. Cheap to copy (shared handle).
class CloudMap {
 public:
  explicit CloudMap(const CloudMapParams& params = CloudMapParams(), size_t max_voxels = (size_t)1 << 20) : params_(params), max_voxels_(max_voxels) {
    loamx_ctx* ctx = gpu::defaultContext();
    loamx_cloud_map_params p;
    loamx_default_cloud_map_params(&p);
    p.leaf = params.leaf, p.min_range = params.min_range, p.max_range = params.max_range;
    loamx_cloud_map* h = nullptr;
    gpu::check(ctx, loamx_cloud_map_create(ctx, &p, max_voxels, &h));
    handle_ = std::shared_ptr<loamx_cloud_map>(h, [](loamx_cloud_map* m) { loamx_cloud_map_destroy(gpu::defaultContext(), m); });
  }
  const CloudMapParams& params() const { return params_; }
  size_t maxVoxels() const { return max_voxels_; }
  /// One cloud in the sensor frame at world_T_sensor. Float fields read through FieldAccessor travel as floats, like the
  /// scans of extractFeatures.
  template <template <typename> class Accessor = FieldAccessor, typename PointType, typename Alloc>
  void add(const std::vector<PointType, Alloc>& points, const Pose3d& world_T_sensor) {
    double pose[7];
    world_T_sensor.toArray(pose);
    addPacked<Accessor>(points, pose);
  }
  /// One cloud that is in the map frame already (no transform)
  template <template <typename> class Accessor = FieldAccessor, typename PointType, typename Alloc>
  void add(const std::vector<PointType, Alloc>& points) {
    addPacked<Accessor>(points, nullptr);
  }
  void clear() {
    loamx_ctx* ctx = gpu::defaultContext();
    gpu::check(ctx, loamx_cloud_map_clear(ctx, handle_.get()));
  }
  /// Removes the voxels outside the box center + [lo, hi] (metres, map frame, widened to voxel boundaries; loamx.h, "map window"):
  /// the map keeps following the sensor at a fixed max_voxels. Infinite bounds are allowed. Synchronises.
  MapCrop crop(const std::array<double, 3>& lo, const std::array<double, 3>& hi, const std::array<double, 3>& center = {0.0, 0.0, 0.0}) {
    return gpu::cropWindow(loamx_cloud_map_crop, handle_.get(), lo, hi, center);
  }
  /// The centroids of the voxels that hold at least min_points points, in order of first appearance
  CloudMapPoints points(uint32_t min_points = 1) const {
    loamx_ctx* ctx = gpu::defaultContext();
    const size_t room = (size_t)stats().voxels;
    CloudMapPoints out;
    out.xyz.resize(3 * room), out.counts.resize(room), out.first.resize(room);
    size_t n = 0;
    gpu::check(ctx, loamx_cloud_map_emit(ctx, handle_.get(), min_points, out.xyz.data(), out.counts.data(), out.first.data(), room, &n));
    n = n < room ? n : room;
    out.xyz.resize(3 * n), out.counts.resize(n), out.first.resize(n);
    return out;
  }
  CloudMapStats stats() const {
    loamx_ctx* ctx = gpu::defaultContext();
    loamx_cloud_map_stats s;
    gpu::check(ctx, loamx_cloud_map_stats_read(ctx, handle_.get(), &s));
    CloudMapStats out;
    out.voxels = s.voxels, out.points_offered = s.points_offered, out.points_used = s.points_used, out.invalid = s.invalid;
    out.range = s.range, out.outside = s.outside, out.overflow = s.overflow;
    return out;
  }
  loamx_cloud_map* handle() const { return handle_.get(); }

 private:
  template <template <typename> class Accessor, typename PointType, typename Alloc>
  void addPacked(const std::vector<PointType, Alloc>& points, const double* pose) {
    loamx_ctx* ctx = gpu::defaultContext();
    if constexpr (gpu::float_scan_v<Accessor, PointType>) {
      const std::vector<float> xyz = gpu::packFloat(points);
      gpu::check(ctx, loamx_cloud_map_add_cloud_f32(ctx, handle_.get(), xyz.data(), 3, points.size(), pose));
    } else {
      const std::vector<double> xyz = gpu::pack<Accessor>(points);
      gpu::check(ctx, loamx_cloud_map_add_cloud(ctx, handle_.get(), xyz.data(), 3, points.size(), pose));
    }
  }

  CloudMapParams params_;
  size_t max_voxels_;
  std::shared_ptr<loamx_cloud_map> handle_;
};

}  // namespace loam
