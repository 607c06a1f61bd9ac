/** @brief Extension (not in the reference): range-image segmentation of an organised scan on the device.
 *
 * The pass LeGO-LOAM and LIO-SAM put in front of the feature extraction: the ground is labelled, the other returns are
 * clustered by connected components of the scan's cylindrical H x W image under an angle criterion, and the components too
 * small to be a surface (leaves, wires, rain, the edges of moving objects) are told from the others. segmentScan returns
 * the class, component and component size of every cell, the accepted components, and a filtered scan to hand to
 * extractFeatures. The rule per cell and per pair of cells is written out in loamx.h ("scan segmentation"); the result does
 * not depend on how the device schedules its threads.
 */
#pragma once
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "common.h"

namespace loam {

/// loamx_segment_params; the defaults are loamx_default_segment_params'
struct SegmentationParams {
  size_t ground_lines = 0;  ///< lines (from line 0) that can be ground; 0: all of them
  double ground_angle = 10.0 * 3.14159265358979323846 / 180.0;   ///< largest slope between two lines of the ground (radians)
  double segment_angle = 60.0 * 3.14159265358979323846 / 180.0;  ///< LeGO-LOAM's segmentation angle (radians)
  size_t min_cluster_points = 30;      ///< a component of at least this many cells is accepted ...
  size_t min_tall_cluster_points = 5;  ///< ... and so is one of at least this many cells
  size_t min_tall_cluster_lines = 3;   ///<     that spans at least this many lines
  bool drop_outliers = true;           ///< the filtered scan leaves out the cells of rejected components
  bool drop_ground = false;            ///< ... and the ground
};

/// Class of a cell
enum class SegmentClass : uint8_t {
  Invalid = LOAMX_SEGMENT_INVALID,  ///< no return, a non-finite coordinate, or out of range
  Ground = LOAMX_SEGMENT_GROUND,
  Cluster = LOAMX_SEGMENT_CLUSTER,  ///< a cell of an accepted component
  Outlier = LOAMX_SEGMENT_OUTLIER   ///< a cell of a rejected component
};

/// An accepted component: its smallest cell index, its number of cells, its first and last line
using SegmentCluster = loamx_segment_cluster;

/// What segmentScan returns; every per-cell vector has scan_lines x points_per_line entries, row-major [line][column]
template <typename PointType, template <typename> class Alloc = std::allocator>
struct ScanSegmentation {
  static constexpr uint32_t kNoLabel = LOAMX_SEGMENT_NO_LABEL;
  std::vector<SegmentClass> classes;
  std::vector<uint32_t> labels;                       ///< the component's smallest cell index for Cluster / Outlier cells, else kNoLabel
  std::vector<uint32_t> sizes;                        ///< the component's number of cells for Cluster / Outlier cells, else 0
  std::vector<PointType, Alloc<PointType>> filtered;  ///< the kept cells copied whole; `empty_point` in the others
  std::vector<SegmentCluster> clusters;               ///< the accepted components by ascending root
  uint32_t invalid = 0, ground = 0, cluster_cells = 0, outlier_cells = 0;  ///< they add up to the scan's size
  uint32_t accepted = 0, rejected = 0, largest = 0;   ///< components accepted / rejected, the size of the largest
};

namespace gpu {
inline loamx_segment_params toC(const SegmentationParams& p) {
  loamx_segment_params c;
  loamx_default_segment_params(&c);
  c.ground_lines = p.ground_lines, c.ground_angle = p.ground_angle, c.segment_angle = p.segment_angle;
  c.min_cluster_points = p.min_cluster_points, c.min_tall_cluster_points = p.min_tall_cluster_points;
  c.min_tall_cluster_lines = p.min_tall_cluster_lines;
  c.drop_outliers = p.drop_outliers ? 1u : 0u, c.drop_ground = p.drop_ground ? 1u : 0u;
  return c;
}
inline int segmentC(loamx_ctx* c, const double* s, const loamx_lidar_params* l, const loamx_segment_params* p, uint8_t* cl, uint32_t* la,
                    uint32_t* sz, loamx_segment_cluster* k, size_t cap, uint32_t* st) {
  return loamx_segment_scan(c, s, l, p, cl, la, sz, nullptr, k, cap, st);
}
inline int segmentC(loamx_ctx* c, const float* s, const loamx_lidar_params* l, const loamx_segment_params* p, uint8_t* cl, uint32_t* la,
                    uint32_t* sz, loamx_segment_cluster* k, size_t cap, uint32_t* st) {
  return loamx_segment_scan_f32(c, s, l, p, cl, la, sz, nullptr, k, cap, st);
}
}  // namespace gpu

/** @brief Segments an organised scan. The coordinates are read through the Accessor (float fields read through FieldAccessor
 * travel as floats, like the scans of extractFeatures). A kept cell of the filtered scan is the input point copied WHOLE, so
 * whatever else the point type carries comes along; a dropped cell holds `empty_point`, which must read as (0, 0, 0) for the
 * extraction to take it for a beam without a return. Throws like extractFeatures on a scan of the wrong size and on parameters
 * the C ABI refuses. */
template <template <typename> class Accessor = FieldAccessor, typename PointType, template <typename> class Alloc>
ScanSegmentation<PointType, Alloc> segmentScan(const std::vector<PointType, Alloc<PointType>>& input_scan, const LidarParams& lidar_params,
                                               const SegmentationParams& params, const PointType& empty_point) {
  validateLidarScan(input_scan, lidar_params);
  ScanSegmentation<PointType, Alloc> out;
  const size_t n = input_scan.size();
  loamx_ctx* ctx = gpu::defaultContext();
  const loamx_lidar_params lp = gpu::toC(lidar_params);
  const loamx_segment_params sp = gpu::toC(params);
  std::vector<uint8_t> classes(n);
  out.labels.assign(n, ScanSegmentation<PointType, Alloc>::kNoLabel), out.sizes.assign(n, 0u);
  out.clusters.resize(n);
  uint32_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if constexpr (gpu::float_scan_v<Accessor, PointType>) {
    const std::vector<float> xyz = gpu::packFloat(input_scan);
    gpu::check(ctx, gpu::segmentC(ctx, xyz.data(), &lp, &sp, classes.data(), out.labels.data(), out.sizes.data(), out.clusters.data(), n, st));
  } else {
    const std::vector<double> xyz = gpu::pack<Accessor>(input_scan);
    gpu::check(ctx, gpu::segmentC(ctx, xyz.data(), &lp, &sp, classes.data(), out.labels.data(), out.sizes.data(), out.clusters.data(), n, st));
  }
  out.clusters.resize(st[7]);
  out.invalid = st[0], out.ground = st[1], out.cluster_cells = st[2], out.outlier_cells = st[3];
  out.accepted = st[4], out.rejected = st[5], out.largest = st[6];
  out.classes.resize(n);
  out.filtered.assign(n, empty_point);
  for (size_t i = 0; i < n; i++) {
    const SegmentClass c = static_cast<SegmentClass>(classes[i]);
    out.classes[i] = c;
    if (c == SegmentClass::Cluster || (c == SegmentClass::Outlier && !params.drop_outliers) || (c == SegmentClass::Ground && !params.drop_ground))
      out.filtered[i] = input_scan[i];
  }
  return out;
}
/// the same with a value-initialised point in the dropped cells (zero for plain structs and for mini_eigen vectors)
template <template <typename> class Accessor = FieldAccessor, typename PointType, template <typename> class Alloc>
ScanSegmentation<PointType, Alloc> segmentScan(const std::vector<PointType, Alloc<PointType>>& input_scan, const LidarParams& lidar_params,
                                               const SegmentationParams& params = SegmentationParams()) {
  return segmentScan<Accessor>(input_scan, lidar_params, params, PointType());
}

}  // namespace loam
