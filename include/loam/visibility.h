/** @brief Extension (not in the reference): map cleaning by visibility votes on the device.
 *
 * A cloud map keeps everything the sensor ever hit, a passing car included. visibilityVotes asks, for every pair of a map
 * point and a scan, whether the beam that looked towards the point stopped at it (agree), stopped before it (occluded), passed
 * through it (through) or returned nothing there (empty); removeDynamicPoints takes the points that many scans saw through and
 * few confirmed out of the map, keeping the others in their order. The rule per pair is written out in loamx.h ("map
 * cleaning"); the votes are integer counts and do not depend on how the device schedules its threads.
 */
#pragma once
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "common.h"
#include "geometry.h"
#include "organize.h"

namespace loam {

/// loamx_visibility_params; the defaults are loamx_default_visibility_params'
struct VisibilityParams {
  double min_range = 1.0;     ///< a scan votes on the points between min_range ...
  double max_range = 80.0;    ///< ... and max_range of its sensor; scan cells nearer than min_range are no returns
  double margin = 0.3;        ///< a return within margin + margin_rel * range of the point's range agrees with it
  double margin_rel = 0.01;
  uint32_t window_lines = 1;  ///< cells looked at around the point's own: this many lines up and down ...
  uint32_t window_cols = 1;   ///< ... and this many columns each way (at most 3 each)
  uint32_t min_through = 2;   ///< a point is dynamic iff through >= min_through ...
  double through_ratio = 1.0; ///< ... and through >= through_ratio * agree
};

/// The votes of one map point: the scans with each verdict
using VisibilityVotes = loamx_visibility_tally;

/// What removeDynamicPoints returns
template <typename PointType, typename Alloc = std::allocator<PointType>>
struct CleanedMap {
  std::vector<uint8_t> dynamic;                 ///< per input point: 1 = dynamic
  std::vector<uint32_t> static_index;           ///< the indices of the points that stay, ascending
  std::vector<PointType, Alloc> static_points;  ///< those points, copied whole
};

namespace gpu {
inline loamx_visibility_params toC(const VisibilityParams& p) {
  loamx_visibility_params c;
  loamx_default_visibility_params(&c);
  c.min_range = p.min_range, c.max_range = p.max_range, c.margin = p.margin, c.margin_rel = p.margin_rel;
  c.window_lines = p.window_lines, c.window_cols = p.window_cols, c.min_through = p.min_through, c.through_ratio = p.through_ratio;
  return c;
}
inline int visibilityVotesC(loamx_ctx* c, const loamx_scan_layout* l, const double* m, size_t n, const double* s, size_t ns, const double* poses,
                            const loamx_visibility_params* p, loamx_visibility_tally* v) {
  return loamx_visibility_votes(c, l, m, 3, n, s, ns, poses, p, v);
}
inline int visibilityVotesC(loamx_ctx* c, const loamx_scan_layout* l, const double* m, size_t n, const float* s, size_t ns, const double* poses,
                            const loamx_visibility_params* p, loamx_visibility_tally* v) {
  return loamx_visibility_votes_f32(c, l, m, 3, n, s, ns, poses, p, v);
}
/// a device allocation that frees itself
struct DeviceBlock {
  loamx_ctx* ctx;
  void* p = nullptr;
  DeviceBlock(loamx_ctx* c, size_t bytes) : ctx(c) { check(ctx, loamx_dev_alloc(ctx, bytes ? bytes : 8, &p)); }
  ~DeviceBlock() {
    if (p) loamx_dev_free(ctx, p);
  }
  DeviceBlock(const DeviceBlock&) = delete;
  DeviceBlock& operator=(const DeviceBlock&) = delete;
};
}  // namespace gpu

/** @brief The votes of map_points (world frame; their coordinates travel as doubles) over organised scans of the layout's shape
 * taken at world_T_scan. All coordinates are read through the Accessor (the scans' float fields read through FieldAccessor travel
 * as floats, like the scans of extractFeatures). Throws on a scan of the wrong size, on a pose count that differs from the scan
 * count and on parameters the C ABI refuses. */
template <template <typename> class Accessor = FieldAccessor, typename MapPoint, typename MapAlloc, typename PointType, typename Alloc>
std::vector<VisibilityVotes> visibilityVotes(const std::vector<MapPoint, MapAlloc>& map_points,
                                             const std::vector<std::vector<PointType, Alloc>>& scans, const std::vector<Pose3d>& world_T_scan,
                                             const ScanLayout& layout, const VisibilityParams& params = VisibilityParams()) {
  if (scans.size() != world_T_scan.size()) throw std::runtime_error("visibilityVotes: as many poses as scans are needed");
  const size_t cells = layout.scanLines() * layout.pointsPerLine();
  for (const auto& s : scans)
    if (s.size() != cells) throw std::runtime_error("visibilityVotes: a scan does not have the layout's size");
  loamx_ctx* ctx = gpu::defaultContext();
  const loamx_visibility_params vp = gpu::toC(params);
  const std::vector<double> m = gpu::pack<Accessor>(map_points);
  std::vector<double> poses(7 * scans.size());
  for (size_t i = 0; i < scans.size(); i++) world_T_scan[i].toArray(poses.data() + 7 * i);
  std::vector<VisibilityVotes> votes(map_points.size(), VisibilityVotes{0, 0, 0, 0});
  if constexpr (gpu::float_scan_v<Accessor, PointType>) {
    std::vector<float> xyz;
    xyz.reserve(3 * cells * scans.size());
    for (const auto& s : scans) {
      const std::vector<float> one = gpu::packFloat(s);
      xyz.insert(xyz.end(), one.begin(), one.end());
    }
    gpu::check(ctx, gpu::visibilityVotesC(ctx, layout.handle(), m.data(), map_points.size(), xyz.data(), scans.size(), poses.data(), &vp, votes.data()));
  } else {
    std::vector<double> xyz;
    xyz.reserve(3 * cells * scans.size());
    for (const auto& s : scans) {
      const std::vector<double> one = gpu::pack<Accessor>(s);
      xyz.insert(xyz.end(), one.begin(), one.end());
    }
    gpu::check(ctx, gpu::visibilityVotesC(ctx, layout.handle(), m.data(), map_points.size(), xyz.data(), scans.size(), poses.data(), &vp, votes.data()));
  }
  return votes;
}

/** @brief The decision over the votes (loamx_visibility_filter_dev on uploaded copies): which points are dynamic, and the others
 * in their input order. Throws when votes and map_points differ in size and on parameters the C ABI refuses. */
template <typename MapPoint, typename MapAlloc>
CleanedMap<MapPoint, MapAlloc> removeDynamicPoints(const std::vector<MapPoint, MapAlloc>& map_points, const std::vector<VisibilityVotes>& votes,
                                                   const VisibilityParams& params = VisibilityParams()) {
  if (votes.size() != map_points.size()) throw std::runtime_error("removeDynamicPoints: one record of votes per map point is needed");
  loamx_ctx* ctx = gpu::defaultContext();
  const loamx_visibility_params vp = gpu::toC(params);
  const size_t n = votes.size();
  CleanedMap<MapPoint, MapAlloc> out;
  out.dynamic.assign(n, 0);
  gpu::DeviceBlock d_votes(ctx, n * sizeof(VisibilityVotes)), d_dyn(ctx, n), d_index(ctx, n * sizeof(uint32_t)), d_n(ctx, sizeof(uint32_t));
  if (n) gpu::check(ctx, loamx_copy_to_device(ctx, d_votes.p, votes.data(), n * sizeof(VisibilityVotes)));
  gpu::check(ctx, loamx_visibility_filter_dev(ctx, static_cast<const loamx_visibility_tally*>(d_votes.p), n, &vp, nullptr, 3, static_cast<uint8_t*>(d_dyn.p),
                                              nullptr, static_cast<uint32_t*>(d_index.p), n, static_cast<uint32_t*>(d_n.p)));
  uint32_t kept = 0;
  gpu::check(ctx, loamx_copy_to_host(ctx, &kept, d_n.p, sizeof(kept)));
  out.static_index.resize(kept);
  if (n) gpu::check(ctx, loamx_copy_to_host(ctx, out.dynamic.data(), d_dyn.p, n));
  if (kept) gpu::check(ctx, loamx_copy_to_host(ctx, out.static_index.data(), d_index.p, kept * sizeof(uint32_t)));
  out.static_points.reserve(kept);
  for (uint32_t i : out.static_index) out.static_points.push_back(map_points[i]);
  return out;
}

}  // namespace loam
