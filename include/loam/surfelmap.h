/** @brief Extension (not in the reference): the surfel map on the device, per voxel the mean, the covariance and the normal.
 *
 * A SurfelMap takes scans (or any clouds) at their poses like a CloudMap and keeps, per voxel, integer first and second moments
 * and a sum of the directions back to the sensor. It reads out one Surfel per voxel in order of first appearance: mean,
 * covariance, eigenvalues ascending, and the unit normal turned towards where the voxel was seen from; query() looks up the
 * surfel of a point and its signed distance to the surfel's plane. The sums are integers, so the map does not depend on how the
 * device schedules its threads. The rule is written out in loamx.h ("surfel map").
 */
#pragma once
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <vector>

#include "common.h"
#include "geometry.h"

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
  loamx_surfel_map* handle() const { return handle_.get(); }

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
};

}  // namespace loam
