// test_distance_shim.cpp — loam::OccupancyMap::distanceBox / distanceSlice (include/loam/occupancy.h) through the C++ headers: the
// squared distances, offsets and metres are the C ABI's (loamx_occupancy_distance_box_host / _slice_host on a map of its own that
// took the same clouds), under both settings of unknown_is_obstacle. The C ABI's bytes are compared with the numpy model by
// tests/test_gpu_distance.py. Built and run by tests/test_gpu_distance_modules.py (needs a GPU).
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "loam/loam.h"

using namespace loam;

static int g_failures = 0, g_checks = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    g_checks++;                                                            \
    if (!(cond)) {                                                         \
      g_failures++;                                                        \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
    }                                                                      \
  } while (0)

struct PointD {
  double x, y, z;
};

static std::vector<PointD> scan(uint64_t pair, uint32_t which) {
  const uint32_t H = 16, W = 240, n = H * W;
  std::vector<double> xyz(n * 3);
  loamx_synth_scan_host(7, pair, which, H, W, 0.01, xyz.data());
  std::vector<PointD> out;
  for (uint32_t i = 0; i < n; i++) out.push_back(PointD{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]});
  return out;
}

// the header's field against the C ABI's, byte for byte; returns how many entries are 0 / between 0 and FAR / FAR
static std::array<size_t, 3> compare(OccupancyMap& map, loamx_ctx* ctx, loamx_occupancy_map* cmap, const DistanceParams& params, bool slice) {
  const std::array<int32_t, 3> vmin = {-30, -30, -2};
  const std::array<uint32_t, 3> dims = {60, 60, 5};
  const size_t n = (size_t)dims[0] * dims[1] * (slice ? 1 : dims[2]), axes = slice ? 2 : 3;
  const DistanceField f = slice ? map.distanceSlice(vmin, dims, params) : map.distanceBox(vmin, dims, params);
  loamx_distance_params cp;
  loamx_default_distance_params(&cp);
  cp.max_dist_voxels = params.max_dist_voxels, cp.unknown_is_obstacle = params.unknown_is_obstacle ? 1u : 0u;
  std::vector<uint16_t> d2(n);
  std::vector<int16_t> offset(axes * n);
  std::vector<float> metres(n);
  CHECK((slice ? loamx_occupancy_distance_slice_host : loamx_occupancy_distance_box_host)(ctx, cmap, vmin.data(), dims.data(), &cp, d2.data(),
                                                                                           offset.data(), metres.data()) == LOAMX_OK);
  CHECK(f.size() == n && f.axes == axes && f.offset.size() == axes * n && f.metres.size() == n);
  CHECK(std::memcmp(d2.data(), f.d2.data(), n * sizeof(uint16_t)) == 0);
  CHECK(std::memcmp(offset.data(), f.offset.data(), axes * n * sizeof(int16_t)) == 0);
  CHECK(std::memcmp(metres.data(), f.metres.data(), n * sizeof(float)) == 0);
  std::array<size_t, 3> seen = {0, 0, 0};
  bool consistent = true;
  for (size_t i = 0; i < n; i++) {
    const uint16_t d = f.d2[i];
    seen[d == 0 ? 0 : d == DistanceField::FAR ? 2 : 1]++;
    uint32_t sum = 0;
    for (size_t a = 0; a < axes; a++) sum += (uint32_t)((int32_t)f.offset[axes * i + a] * (int32_t)f.offset[axes * i + a]);
    if (d == DistanceField::FAR) consistent = consistent && sum == 0 && std::isinf(f.metres[i]);
    else consistent = consistent && sum == d && f.metres[i] == (float)(std::sqrt((double)d) * map.params().leaf);
  }
  CHECK(consistent);  // the offset's squared length is d2, and the metres are its root times the leaf
  return seen;
}

int main() {
  DistanceParams dp;
  loamx_distance_params cdp;
  loamx_default_distance_params(&cdp);
  CHECK(dp.max_dist_voxels == cdp.max_dist_voxels && dp.max_dist_voxels == 10 && !dp.unknown_is_obstacle && cdp.unknown_is_obstacle == 0);
  CHECK(DistanceField::FAR == 0xFFFF);

  OccupancyParams params;
  loamx_occupancy_params cp;
  loamx_default_occupancy_params(&cp);
  params.leaf = cp.leaf = 0.5;
  params.max_range = cp.max_range = 30.0;
  OccupancyMap map(params, 1 << 17);
  loamx_ctx* ctx = gpu::defaultContext();
  loamx_occupancy_map* cmap = nullptr;
  CHECK(loamx_occupancy_create(ctx, &cp, 1 << 17, &cmap) == LOAMX_OK);

  std::array<size_t, 3> seen = compare(map, ctx, cmap, dp, false);  // both empty
  CHECK(seen[0] == 0 && seen[1] == 0);
  for (uint64_t place = 0; place < 2; place++) {
    const std::vector<PointD> pts = scan(place, 0);
    const std::vector<double> xyz = gpu::pack<FieldAccessor>(pts);
    double p7[7];
    loamx_synth_pair_pose(7, place, p7);
    const Pose3d pose = Pose3d::fromArray(p7);
    double back[7];
    pose.toArray(back);
    map.add(pts, pose);
    CHECK(loamx_occupancy_add_cloud(ctx, cmap, xyz.data(), 3, pts.size(), back) == LOAMX_OK);
  }
  for (int unknown = 0; unknown < 2; unknown++) {
    for (uint32_t R : {3u, 10u}) {
      dp.max_dist_voxels = R, dp.unknown_is_obstacle = unknown != 0;
      seen = compare(map, ctx, cmap, dp, false);
      CHECK(seen[0] > 50 && seen[1] > 1000);
      seen = compare(map, ctx, cmap, dp, true);
      CHECK(seen[0] > 20 && seen[1] > 100);
    }
  }

  bool threw = false;
  try {
    dp.max_dist_voxels = 0;
    map.distanceBox({0, 0, 0}, {2, 2, 2}, dp);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);
  threw = false;
  try {
    dp.max_dist_voxels = 256;
    map.distanceSlice({0, 0, 0}, {2, 2, 2}, dp);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);

  loamx_occupancy_destroy(ctx, cmap);
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
