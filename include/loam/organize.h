/** @brief Extension (not in the reference): unordered point clouds into organised scans on the device.
 *
 * The reference demands an organised scan — scan_lines x points_per_line points, row-major [line][column]
 * (common.h:104-113) — and leaves the projection to its users. Sensor drivers and datasets deliver unordered x, y, z
 * (with or without a ring number), with dropped returns missing and, for dual-return sensors, two points per beam.
 * ScanLayout describes the grid (azimuth of column 0, sense of rotation, the beams' elevations, an optional ring map);
 * organizeCloud puts a cloud into it with a winner per cell that does not depend on how the device schedules its threads.
 * The rule per point is written out in loamx.h ("unordered clouds into scans").
 */
#pragma once
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <vector>

#include "common.h"

namespace loam {

/// The winner among the points of a cloud that land in one cell
enum class OrganizeKeep : uint32_t {
  First = LOAMX_ORGANIZE_KEEP_FIRST,     ///< the lowest input index
  Nearest = LOAMX_ORGANIZE_KEEP_NEAREST  ///< the smallest range; on equal ranges the lowest index
};

/// loamx_organize_params with owned arrays; the defaults are loamx_default_organize_params'
struct OrganizeParams {
  double azimuth_zero = 0.0;       ///< azimuth of the centre of column 0 (radians)
  bool clockwise = false;          ///< columns counted clockwise seen from +z
  OrganizeKeep keep = OrganizeKeep::First;
  std::vector<double> elevations;  ///< scan_lines ascending beam elevations (radians); empty: linear fov_bottom .. fov_top
  double fov_bottom = -15.0 * 3.14159265358979323846 / 180.0;
  double fov_top = 15.0 * 3.14159265358979323846 / 180.0;
  std::vector<uint16_t> ring_map;  ///< ring number -> line (0xFFFF: drop the ring); empty: the ring number is the line
};

/// The grid of a sensor with its two boundary tables on the device (loamx_scan_layout). Cheap to copy (shared handle).
class ScanLayout {
 public:
  explicit ScanLayout(const LidarParams& lidar, const OrganizeParams& params = OrganizeParams())
      : scan_lines_(lidar.scan_lines), points_per_line_(lidar.points_per_line) {
    if (!params.elevations.empty() && params.elevations.size() != lidar.scan_lines)
      throw std::runtime_error("loam::ScanLayout: the number of elevations does not match scan_lines");
    loamx_ctx* ctx = gpu::defaultContext();
    loamx_organize_params p;
    loamx_default_organize_params(&p);
    p.azimuth_zero = params.azimuth_zero, p.clockwise = params.clockwise ? 1u : 0u, p.keep = static_cast<uint32_t>(params.keep);
    p.elevations = params.elevations.empty() ? nullptr : params.elevations.data();
    p.fov_bottom = params.fov_bottom, p.fov_top = params.fov_top;
    p.ring_map = params.ring_map.empty() ? nullptr : params.ring_map.data(), p.n_ring_map = params.ring_map.size();
    const loamx_lidar_params lp = gpu::toC(lidar);
    loamx_scan_layout* h = nullptr;
    gpu::check(ctx, loamx_scan_layout_create(ctx, &lp, &p, &h));
    handle_ = std::shared_ptr<loamx_scan_layout>(h, [](loamx_scan_layout* l) { loamx_scan_layout_destroy(gpu::defaultContext(), l); });
  }
  size_t scanLines() const { return scan_lines_; }
  size_t pointsPerLine() const { return points_per_line_; }
  size_t cells() const { return scan_lines_ * points_per_line_; }
  /// u_k = (cos phi_k, sin phi_k) of the column boundaries, points_per_line x 2, exactly as the kernels use them
  std::vector<double> columnDirections() const {
    std::vector<double> v(2 * points_per_line_);
    loamx_scan_layout_tables(handle_.get(), v.data(), nullptr);
    return v;
  }
  /// the scan_lines + 1 tangents of the line boundaries, exactly as the kernels use them
  std::vector<double> lineTangents() const {
    std::vector<double> v(scan_lines_ + 1);
    loamx_scan_layout_tables(handle_.get(), nullptr, v.data());
    return v;
  }
  const loamx_scan_layout* handle() const { return handle_.get(); }

 private:
  size_t scan_lines_, points_per_line_;
  std::shared_ptr<loamx_scan_layout> handle_;
};

/// What organizeCloud returns: the scan (cells() points, row-major [line][column]), the index map and the four counters
template <typename PointType, template <typename> class Alloc = std::allocator>
struct OrganizedCloud {
  static constexpr uint32_t kNoPoint = 0xFFFFFFFFu;
  std::vector<PointType, Alloc<PointType>> scan;  ///< the winner of every cell, copied whole; `empty_point` where there is none
  std::vector<uint32_t> src_idx;                  ///< index of the winner in the input cloud, or kNoPoint
  uint32_t filled = 0, invalid = 0, outside = 0, collisions = 0;  ///< they add up to the cloud's size
};

namespace gpu {
inline int organizeC(loamx_ctx* c, const loamx_scan_layout* l, const double* p, const uint16_t* r, size_t n, double* s, uint32_t* i, uint32_t* st) {
  return loamx_organize_cloud(c, l, p, 3, r, n, s, i, st);
}
inline int organizeC(loamx_ctx* c, const loamx_scan_layout* l, const float* p, const uint16_t* r, size_t n, float* s, uint32_t* i, uint32_t* st) {
  return loamx_organize_cloud_f32(c, l, p, 3, r, n, s, i, st);
}
template <typename T>
void organizeIndices(const ScanLayout& layout, const std::vector<T>& xyz, const std::vector<uint16_t>& rings, std::vector<uint32_t>& src_idx,
                     uint32_t stats[4]) {
  const size_t n = xyz.size() / 3;
  if (!rings.empty() && rings.size() != n) throw std::runtime_error("loam::organizeCloud: one ring number per point, or none");
  std::vector<T> scan(layout.cells() * 3);
  src_idx.assign(layout.cells(), 0xFFFFFFFFu);
  loamx_ctx* ctx = defaultContext();
  check(ctx, organizeC(ctx, layout.handle(), xyz.data(), rings.empty() ? nullptr : rings.data(), n, scan.data(), src_idx.data(), stats));
}
}  // namespace gpu

/** @brief Puts an unordered cloud into the layout's grid. The coordinates are read through the Accessor (float fields read
 * through FieldAccessor travel as floats, like the scans of extractFeatures); the winner of a cell is copied WHOLE from the
 * input, so whatever else the point type carries (intensity, time stamp) comes along. A cell without a winner holds
 * `empty_point`, which must read as (0, 0, 0) for the extraction to take it for a beam without a return.
 * @param rings one ring number per point, or empty: lines by elevation */
template <template <typename> class Accessor = FieldAccessor, typename PointType, template <typename> class Alloc>
OrganizedCloud<PointType, Alloc> organizeCloud(const std::vector<PointType, Alloc<PointType>>& points, const ScanLayout& layout,
                                                const std::vector<uint16_t>& rings, const PointType& empty_point) {
  OrganizedCloud<PointType, Alloc> out;
  uint32_t stats[4] = {0, 0, 0, 0};
  if constexpr (gpu::float_scan_v<Accessor, PointType>) gpu::organizeIndices(layout, gpu::packFloat(points), rings, out.src_idx, stats);
  else gpu::organizeIndices(layout, gpu::pack<Accessor>(points), rings, out.src_idx, stats);
  out.filled = stats[0], out.invalid = stats[1], out.outside = stats[2], out.collisions = stats[3];
  out.scan.assign(layout.cells(), empty_point);
  for (size_t c = 0; c < out.src_idx.size(); c++)
    if (out.src_idx[c] != OrganizedCloud<PointType, Alloc>::kNoPoint) out.scan[c] = points[out.src_idx[c]];
  return out;
}
/// the same with a value-initialised point in the empty cells (zero for plain structs and for mini_eigen vectors)
template <template <typename> class Accessor = FieldAccessor, typename PointType, template <typename> class Alloc>
OrganizedCloud<PointType, Alloc> organizeCloud(const std::vector<PointType, Alloc<PointType>>& points, const ScanLayout& layout,
                                                const std::vector<uint16_t>& rings = std::vector<uint16_t>()) {
  return organizeCloud<Accessor>(points, layout, rings, PointType());
}

}  // namespace loam
