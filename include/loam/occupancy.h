/** @brief Extension (not in the reference): the occupancy map on the device, free space by ray traversal.
 *
 * An OccupancyMap takes scans (or any clouds) at their poses and walks every beam from the sensor to its return through a voxel
 * grid: the voxel of the return counts a hit, every voxel in front of it a pass. A voxel is then occupied, free or unknown
 * (never seen), the distinction OctoMap provides. The counts are integers, so the map does not depend on how the device
 * schedules its threads or on how a drive is split into calls. It is read per point, as a dense box of voxels, or as the 2-D
 * grid a planner takes. The rule is written out in loamx.h ("occupancy map"). castRays and renderScans ask what a ray through the
 * map meets first, and what scan the map predicts at a pose (loamx.h, "occupancy ray casting").
 */
#pragma once
#include <array>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <vector>

#include "common.h"
#include "geometry.h"

namespace loam {

/// LOAMX_OCC_*: the state of a voxel
enum class Occupancy : uint8_t { UNKNOWN = 0, FREE = 1, OCCUPIED = 2 };

/// loamx_occupancy_params; the defaults are loamx_default_occupancy_params'
struct OccupancyParams {
  double leaf = 0.2;        ///< voxel edge
  double min_range = 0.5;   ///< returns nearer to the sensor are dropped (the all-zero cells of an organised scan among them)
  double max_range = 80.0;  ///< returns farther away make no hit; with clip_long their beam is walked up to this range
  double end_margin = 0.2;  ///< a walk stops this far in front of its return
  bool clip_long = true;
  uint32_t min_hits = 1;    ///< occupied: hits >= min_hits and hits >= occ_ratio x passes
  double occ_ratio = 0.0;   ///< 0: a hit always wins; raise it to let passes erase hits
  uint32_t min_passes = 1;  ///< free: not occupied and passes >= min_passes
};

/// loamx_occupancy_stats
struct OccupancyStats {
  uint64_t rays_offered = 0, rays_hit = 0, invalid = 0, range_short = 0, range_long = 0, outside = 0, visits = 0, voxels = 0, overflow = 0;
};

/// What OccupancyMap::query and ::box return: counts[2 i] hits and counts[2 i + 1] passes of entry i, states[i] its state
struct OccupancyCells {
  std::vector<uint32_t> counts;
  std::vector<uint8_t> states;
  size_t size() const { return states.size(); }
  Occupancy state(size_t i) const { return static_cast<Occupancy>(states[i]); }
};

/// loamx_distance_params; the defaults are loamx_default_distance_params'
struct DistanceParams {
  uint32_t max_dist_voxels = 10;     ///< the cap R in voxels, 1 .. 255: no obstacle within it reads FAR
  bool unknown_is_obstacle = false;  ///< voxels never seen count as obstacles
};

/// What OccupancyMap::distanceBox and ::distanceSlice return (loamx.h, "occupancy distance field"): per entry the squared
/// distance in voxels to the nearest obstacle (FAR beyond the cap), the offset to that obstacle in voxels (`axes` int16 per entry:
/// 3 for a box, 2 for a slice; zeros where d2 is 0 or FAR) and the distance in metres (+inf for FAR)
struct DistanceField {
  static constexpr uint16_t FAR = LOAMX_DIST_FAR;
  size_t axes = 3;
  std::vector<uint16_t> d2;
  std::vector<int16_t> offset;
  std::vector<float> metres;
  size_t size() const { return d2.size(); }
};

/// loamx_raycast_params; the defaults are loamx_default_raycast_params'
struct RaycastParams {
  enum HitAt : uint32_t { AT_ENTER = LOAMX_RAY_AT_ENTER, AT_MIDDLE = LOAMX_RAY_AT_MIDDLE };
  uint32_t skip_start = 0;        ///< visits at the start of a ray that are walked but not tested (a ray that starts on a surface)
  bool unknown_stops = false;     ///< a voxel never seen stops the ray (status UNKNOWN); otherwise it is counted and passed
  uint32_t max_steps = 3 * 4098;  ///< the step cap, at most 2^22: a longer walk ends TRUNCATED
  HitAt hit_at = AT_MIDDLE;       ///< renderScans only: the return lies where the beam enters the hit voxel, or half way through it
};

/// loamx_ray_record (loamx.h, "occupancy ray casting"): what a ray met first
struct RayRecord {
  enum Status : uint32_t {
    CLEAR = LOAMX_RAY_CLEAR, HIT = LOAMX_RAY_HIT, UNKNOWN = LOAMX_RAY_UNKNOWN, TRUNCATED = LOAMX_RAY_TRUNCATED, OUTSIDE = LOAMX_RAY_OUTSIDE,
    INVALID = LOAMX_RAY_INVALID
  };
  uint32_t status = CLEAR;
  uint32_t visits = 0;                   ///< voxels visited, the last one included
  std::array<int32_t, 3> voxel{0, 0, 0};  ///< the voxel the ray stopped or ended in
  uint32_t n_unknown = 0;
  double t_enter = 0.0, t_exit = 0.0;    ///< the parameters in [0, 1] at which the segment enters and leaves that voxel
  bool hit() const { return status == HIT; }
};
static_assert(sizeof(RayRecord) == sizeof(loamx_ray_record), "RayRecord is loamx_ray_record");

/// What OccupancyMap::renderScans returns: per pose and beam (entry pose n_beams + beam) the point in the sensor frame (packed
/// x y z; (0, 0, 0) where nothing is hit: the "no return" cell of an organised scan), the range and the record
struct RenderedScans {
  size_t n_poses = 0, n_beams = 0;
  std::vector<double> xyz;
  std::vector<double> ranges;
  std::vector<RayRecord> records;
};

/// The map (loamx_occupancy_map): table and counters on the device. Cheap to copy (shared handle).
class OccupancyMap {
 public:
  explicit OccupancyMap(const OccupancyParams& params = OccupancyParams(), size_t max_voxels = (size_t)1 << 20)
      : params_(params), max_voxels_(max_voxels) {
    loamx_ctx* ctx = gpu::defaultContext();
    loamx_occupancy_params p;
    loamx_default_occupancy_params(&p);
    p.leaf = params.leaf, p.min_range = params.min_range, p.max_range = params.max_range, p.end_margin = params.end_margin;
    p.clip_long = params.clip_long ? 1u : 0u, p.min_hits = params.min_hits, p.occ_ratio = params.occ_ratio, p.min_passes = params.min_passes;
    loamx_occupancy_map* h = nullptr;
    gpu::check(ctx, loamx_occupancy_create(ctx, &p, max_voxels, &h));
    handle_ = std::shared_ptr<loamx_occupancy_map>(h, [](loamx_occupancy_map* m) { loamx_occupancy_destroy(gpu::defaultContext(), m); });
  }
  const OccupancyParams& params() const { return params_; }
  size_t maxVoxels() const { return max_voxels_; }
  /// One cloud in the sensor frame at world_T_sensor: its beams start at the pose's translation. Float fields read through
  /// FieldAccessor travel as floats, like the scans of extractFeatures.
  template <template <typename> class Accessor = FieldAccessor, typename PointType, typename Alloc>
  void add(const std::vector<PointType, Alloc>& points, const Pose3d& world_T_sensor) {
    double pose[7];
    world_T_sensor.toArray(pose);
    addPacked<Accessor>(points, pose);
  }
  /// One cloud whose sensor stands at the map's origin (no transform)
  template <template <typename> class Accessor = FieldAccessor, typename PointType, typename Alloc>
  void add(const std::vector<PointType, Alloc>& points) {
    addPacked<Accessor>(points, nullptr);
  }
  void clear() {
    loamx_ctx* ctx = gpu::defaultContext();
    gpu::check(ctx, loamx_occupancy_clear(ctx, handle_.get()));
  }
  /// Removes the voxels outside the box center + [lo, hi] (metres, map frame, widened to voxel boundaries; loamx.h, "map window"):
  /// the map keeps following the sensor at a fixed max_voxels. Infinite bounds are allowed. Synchronises.
  MapCrop crop(const std::array<double, 3>& lo, const std::array<double, 3>& hi, const std::array<double, 3>& center = {0.0, 0.0, 0.0}) {
    return gpu::cropWindow(loamx_occupancy_crop, handle_.get(), lo, hi, center);
  }
  /// Counts and state of the voxel of each point (map frame, packed x y z)
  OccupancyCells query(const std::vector<double>& xyz) const {
    loamx_ctx* ctx = gpu::defaultContext();
    const size_t n = xyz.size() / 3;
    OccupancyCells out;
    out.counts.resize(2 * n), out.states.resize(n);
    gpu::check(ctx, loamx_occupancy_query(ctx, handle_.get(), xyz.data(), 3, n, out.counts.data(), out.states.data()));
    return out;
  }
  /// The voxels vmin .. vmin + dims - 1, x fastest: entry (z dims[1] + y) dims[0] + x
  OccupancyCells box(const std::array<int32_t, 3>& vmin, const std::array<uint32_t, 3>& dims) const {
    loamx_ctx* ctx = gpu::defaultContext();
    const size_t n = (size_t)dims[0] * dims[1] * dims[2];
    OccupancyCells out;
    out.counts.resize(2 * n), out.states.resize(n);
    gpu::check(ctx, loamx_occupancy_box(ctx, handle_.get(), vmin.data(), dims.data(), out.counts.data(), out.states.data()));
    return out;
  }
  /// The 2-D grid of the box's columns, entry y dims[0] + x: occupied if any level of the column is, otherwise free if any is
  std::vector<uint8_t> slice(const std::array<int32_t, 3>& vmin, const std::array<uint32_t, 3>& dims) const {
    loamx_ctx* ctx = gpu::defaultContext();
    std::vector<uint8_t> grid((size_t)dims[0] * dims[1]);
    gpu::check(ctx, loamx_occupancy_slice(ctx, handle_.get(), vmin.data(), dims.data(), grid.data()));
    return grid;
  }
  /// The clearance of every voxel of the box: the exact distance to the nearest obstacle voxel of the map, those in a halo of
  /// max_dist_voxels around the box included. The layout is box()'s.
  DistanceField distanceBox(const std::array<int32_t, 3>& vmin, const std::array<uint32_t, 3>& dims, const DistanceParams& params = DistanceParams()) {
    return distance(loamx_occupancy_distance_box_host, vmin, dims, params, (size_t)dims[0] * dims[1] * dims[2], 3);
  }
  /// The 2-D clearance grid of the box's columns, each column an obstacle by the state slice() gives it. The layout is slice()'s.
  DistanceField distanceSlice(const std::array<int32_t, 3>& vmin, const std::array<uint32_t, 3>& dims, const DistanceParams& params = DistanceParams()) {
    return distance(loamx_occupancy_distance_slice_host, vmin, dims, params, (size_t)dims[0] * dims[1], 2);
  }
  /// What each segment origins[i] -> ends[i] (map frame, packed x y z) meets first: OctoMap's castRay, for line-of-sight and
  /// segment-collision checks
  std::vector<RayRecord> castRays(const std::vector<double>& origins, const std::vector<double>& ends, const RaycastParams& params = RaycastParams()) const {
    if (origins.size() != ends.size() || origins.size() % 3) throw std::invalid_argument("castRays: origins and ends are packed x y z of equal length");
    loamx_ctx* ctx = gpu::defaultContext();
    const loamx_raycast_params p = raycastParams(params);
    std::vector<RayRecord> out(origins.size() / 3);
    gpu::check(ctx, loamx_occupancy_cast_rays_host(ctx, handle_.get(), origins.data(), ends.data(), 3, out.size(), &p,
                                                   reinterpret_cast<loamx_ray_record*>(out.data())));
    return out;
  }
  /// The scans the map predicts at the poses (world_T_sensor) for the unit beam directions `dirs` (sensor frame, packed x y z, in
  /// the scan's cell order), out to max_range. The range of a return is a voxel's entry or middle: quantised to the leaf.
  RenderedScans renderScans(const std::vector<double>& dirs, const std::vector<Pose3d>& poses, double max_range,
                            const RaycastParams& params = RaycastParams()) const {
    if (dirs.size() % 3) throw std::invalid_argument("renderScans: dirs is packed x y z");
    loamx_ctx* ctx = gpu::defaultContext();
    const loamx_raycast_params p = raycastParams(params);
    RenderedScans out;
    out.n_poses = poses.size(), out.n_beams = dirs.size() / 3;
    std::vector<double> packed(7 * poses.size());
    for (size_t i = 0; i < poses.size(); i++) poses[i].toArray(packed.data() + 7 * i);
    const size_t n = out.n_poses * out.n_beams;
    out.xyz.resize(3 * n), out.ranges.resize(n), out.records.resize(n);
    gpu::check(ctx, loamx_occupancy_render_scans_host(ctx, handle_.get(), dirs.data(), out.n_beams, packed.data(), out.n_poses, max_range, &p,
                                                      out.xyz.data(), out.ranges.data(), reinterpret_cast<loamx_ray_record*>(out.records.data())));
    return out;
  }
  OccupancyStats stats() const {
    loamx_ctx* ctx = gpu::defaultContext();
    loamx_occupancy_stats s;
    gpu::check(ctx, loamx_occupancy_stats_read(ctx, handle_.get(), &s));
    OccupancyStats out;
    out.rays_offered = s.rays_offered, out.rays_hit = s.rays_hit, out.invalid = s.invalid, out.range_short = s.range_short;
    out.range_long = s.range_long, out.outside = s.outside, out.visits = s.visits, out.voxels = s.voxels, out.overflow = s.overflow;
    return out;
  }
  loamx_occupancy_map* handle() const { return handle_.get(); }

 private:
  static loamx_raycast_params raycastParams(const RaycastParams& params) {
    loamx_raycast_params p;
    loamx_default_raycast_params(&p);
    p.skip_start = params.skip_start, p.unknown_stops = params.unknown_stops ? 1u : 0u, p.max_steps = params.max_steps, p.hit_at = params.hit_at;
    return p;
  }
  template <typename Fn>
  DistanceField distance(Fn fn, const std::array<int32_t, 3>& vmin, const std::array<uint32_t, 3>& dims, const DistanceParams& params, size_t n,
                         size_t axes) {
    loamx_ctx* ctx = gpu::defaultContext();
    loamx_distance_params p;
    loamx_default_distance_params(&p);
    p.max_dist_voxels = params.max_dist_voxels, p.unknown_is_obstacle = params.unknown_is_obstacle ? 1u : 0u;
    DistanceField out;
    out.axes = axes;
    out.d2.resize(n), out.offset.resize(axes * n), out.metres.resize(n);
    gpu::check(ctx, fn(ctx, handle_.get(), vmin.data(), dims.data(), &p, out.d2.data(), out.offset.data(), out.metres.data()));
    return out;
  }
  template <template <typename> class Accessor, typename PointType, typename Alloc>
  void addPacked(const std::vector<PointType, Alloc>& points, const double* pose) {
    loamx_ctx* ctx = gpu::defaultContext();
    if constexpr (gpu::float_scan_v<Accessor, PointType>) {
      const std::vector<float> xyz = gpu::packFloat(points);
      gpu::check(ctx, loamx_occupancy_add_cloud_f32(ctx, handle_.get(), xyz.data(), 3, points.size(), pose));
    } else {
      const std::vector<double> xyz = gpu::pack<Accessor>(points);
      gpu::check(ctx, loamx_occupancy_add_cloud(ctx, handle_.get(), xyz.data(), 3, points.size(), pose));
    }
  }

  OccupancyParams params_;
  size_t max_voxels_;
  std::shared_ptr<loamx_occupancy_map> handle_;
};

}  // namespace loam
