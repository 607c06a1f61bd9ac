// segment_math.h — per-cell and per-pair math of the scan segmentation (loamx.h, "scan segmentation": the rule). __host__ __device__
// so that tests/hostcheck_segment can compare the exact kernel arithmetic bit for bit with the numpy model on the CPU; the product
// only calls it from HIP kernels (segment_kernels.hip). FP64 throughout, every product, sum and difference rounded on its own in
// the order written: must be compiled with -ffp-contract=off, as the other *_math.h headers.
#pragma once
#include <stdint.h>

#include "extract_math.h"

namespace loamx {

// classes of a cell (loamx.h: LOAMX_SEGMENT_*); kSegNode is what the first stage leaves for the cells the later stages decide
enum : uint8_t { kSegInvalid = 0, kSegGround = 1, kSegCluster = 2, kSegOutlier = 3, kSegNode = 2 };
constexpr uint32_t kSegNoLabel = 0xFFFFFFFFu;

// the rule's parameters as the kernels take them (api_segment.hip: make_segment_params)
struct SegParams {
  uint32_t H, W;
  uint32_t G;  // lines that take part in the ground test: ground_lines, or H when that is 0 or larger than H
  double min_range, max_range;
  double tg2, c2;  // tan(ground_angle)^2, cos(segment_angle)^2 (loamx_segment_constants)
  uint32_t min_cluster, min_tall_points, min_tall_lines;
  uint32_t drop_outliers, drop_ground;
};

LOAMX_EHD bool seg_finite(double v) { return v - v == 0.0; }  // false for NaN and for either infinity

// Valid: three finite coordinates and a range the extraction keeps (point_code: r < min_range || r > max_range is out)
LOAMX_EHD bool seg_valid(double x, double y, double z, double min_range, double max_range) {
  if (!(seg_finite(x) && seg_finite(y) && seg_finite(z))) return false;
  const double r = point_range(x, y, z);
  return !(r < min_range || r > max_range);
}

// Ground pair: a = p(l, c), b = p(l + 1, c), both valid. dz dz <= tg2 (dx dx + dy dy)
LOAMX_EHD bool seg_ground_pair(double ax, double ay, double az, double bx, double by, double bz, double tg2) {
  const double dx = bx - ax, dy = by - ay, dz = bz - az;
  return dz * dz <= tg2 * (dx * dx + dy * dy);
}

// Connected: the angle at the farther point between its ray and the chord exceeds segment_angle, without atan2 or sqrt:
// t t < (c2 m) e2 with m the larger squared range, t = m - a.b, e = b - a. Symmetric in a and b to the bit.
LOAMX_EHD bool seg_connected(double ax, double ay, double az, double bx, double by, double bz, double c2) {
  const double r2a = (ax * ax + ay * ay) + az * az;
  const double r2b = (bx * bx + by * by) + bz * bz;
  const double m = r2a > r2b ? r2a : r2b;
  const double dot = (ax * bx + ay * by) + az * bz;
  const double ex = bx - ax, ey = by - ay, ez = bz - az;
  const double e2 = (ex * ex + ey * ey) + ez * ez;
  const double t = m - dot;
  return t * t < (c2 * m) * e2;
}

// accepted: large enough, or tall enough for its size
LOAMX_EHD bool seg_accepted(uint32_t size, uint32_t span, const SegParams& P) {
  return size >= P.min_cluster || (size >= P.min_tall_points && span >= P.min_tall_lines);
}

}  // namespace loamx
