// test_cloudmap_shim.cpp — loam::CloudMap (include/loam/cloudmap.h) through the C++ headers: centroids, counts, `first` and the
// stats are the C ABI's (loamx_cloud_map_add_cloud[_f32] / loamx_cloud_map_emit on the same packed points and a map of its own),
// for double and float points, with and without a pose, before and after clear().
// Built and run by tests/test_gpu_cloudmap_modules.py (needs a GPU).
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
struct PointF {
  float x, y, z, intensity;
};

static std::vector<PointD> scan(uint64_t pair, uint32_t which) {
  const uint32_t H = 16, W = 240, n = H * W;
  std::vector<double> xyz(n * 3);
  loamx_synth_scan_host(7, pair, which, H, W, 0.01, xyz.data());
  std::vector<PointD> out;
  for (uint32_t i = 0; i < n; i++) out.push_back(PointD{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]});
  return out;
}

// the header's map against the C ABI's, byte for byte
static void compare(const CloudMap& map, loamx_ctx* ctx, loamx_cloud_map* cmap, uint32_t min_points) {
  const CloudMapPoints got = map.points(min_points);
  const CloudMapStats s = map.stats();
  loamx_cloud_map_stats cs;
  CHECK(loamx_cloud_map_stats_read(ctx, cmap, &cs) == LOAMX_OK);
  CHECK(s.voxels == cs.voxels && s.points_offered == cs.points_offered && s.points_used == cs.points_used && s.invalid == cs.invalid &&
        s.range == cs.range && s.outside == cs.outside && s.overflow == cs.overflow && s.overflow == 0);
  const size_t room = (size_t)cs.voxels + 1;
  std::vector<double> xyz(3 * room);
  std::vector<uint32_t> counts(room), first(room);
  size_t n = 0;
  CHECK(loamx_cloud_map_emit(ctx, cmap, min_points, xyz.data(), counts.data(), first.data(), room, &n) == LOAMX_OK);
  CHECK(n == got.size() && n <= cs.voxels && got.xyz.size() == 3 * n && got.first.size() == n);
  if (n != got.size()) return;
  CHECK(n == 0 || std::memcmp(xyz.data(), got.xyz.data(), 3 * n * sizeof(double)) == 0);
  CHECK(n == 0 || std::memcmp(counts.data(), got.counts.data(), n * sizeof(uint32_t)) == 0);
  CHECK(n == 0 || std::memcmp(first.data(), got.first.data(), n * sizeof(uint32_t)) == 0);
  for (size_t i = 0; i < n; i++) CHECK(got.counts[i] >= min_points && (i == 0 || got.first[i] > got.first[i - 1]));
}

int main() {
  CloudMapParams params;
  loamx_cloud_map_params cp;
  loamx_default_cloud_map_params(&cp);
  CHECK(params.leaf == 0.2 && params.min_range == 0.5 && params.max_range == 120.0);
  CHECK(cp.leaf == params.leaf && cp.min_range == params.min_range && cp.max_range == params.max_range);

  params.leaf = cp.leaf = 0.5;
  CloudMap map(params, 1 << 14);
  loamx_ctx* ctx = gpu::defaultContext();
  loamx_cloud_map* cmap = nullptr;
  CHECK(loamx_cloud_map_create(ctx, &cp, 1 << 14, &cmap) == LOAMX_OK);
  CHECK(map.maxVoxels() == (1u << 14) && map.params().leaf == 0.5);
  compare(map, ctx, cmap, 1);  // both empty

  for (int round = 0; round < 2; round++) {
    for (uint64_t place = 0; place < 3; place++) {
      const std::vector<PointD> pts = scan(place, 0);
      const std::vector<double> xyz = gpu::pack<FieldAccessor>(pts);
      double p7[7];
      loamx_synth_pair_pose(7, place, p7);
      const Pose3d pose = Pose3d::fromArray(p7);
      double back[7];
      pose.toArray(back);
      if (place == 1) {
        map.add(pts);  // in the map frame already
        CHECK(loamx_cloud_map_add_cloud(ctx, cmap, xyz.data(), 3, pts.size(), nullptr) == LOAMX_OK);
      } else {
        map.add(pts, pose);
        CHECK(loamx_cloud_map_add_cloud(ctx, cmap, xyz.data(), 3, pts.size(), back) == LOAMX_OK);
      }
      std::vector<PointF> ptsf;
      for (const PointD& p : scan(place, 1)) ptsf.push_back(PointF{(float)p.x, (float)p.y, (float)p.z, 1.0f});
      const std::vector<float> xyzf = gpu::packFloat(ptsf);
      map.add(ptsf, pose);
      CHECK(loamx_cloud_map_add_cloud_f32(ctx, cmap, xyzf.data(), 3, ptsf.size(), back) == LOAMX_OK);
    }
    compare(map, ctx, cmap, 1);
    compare(map, ctx, cmap, 3);
    const CloudMapStats s = map.stats();
    CHECK(s.points_offered == 6u * 16u * 240u && s.voxels > 500 && s.points_used > s.voxels);
    CHECK(map.points(0xFFFFFFFFu).size() == 0);
    map.clear();
    CHECK(loamx_cloud_map_clear(ctx, cmap) == LOAMX_OK);
    CHECK(map.stats().voxels == 0 && map.stats().points_offered == 0 && map.points().size() == 0);
  }

  bool threw = false;
  try {
    CloudMapParams bad;
    bad.leaf = 0.0;
    CloudMap refused(bad);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);

  loamx_cloud_map_destroy(ctx, cmap);
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
