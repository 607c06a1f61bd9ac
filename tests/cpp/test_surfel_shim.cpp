// test_surfel_shim.cpp — loam::SurfelMap (include/loam/surfelmap.h) through the C++ headers: the records, the query and the stats
// are the C ABI's (loamx_surfel_map_add_cloud_host[_f32] / loamx_surfel_map_emit_host / loamx_surfel_map_query on the same packed
// points and a map of its own), for double and float points, with and without a pose, before and after clear().
// Built and run by tests/test_gpu_surfel_modules.py (needs a GPU).
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
static void compare(const SurfelMap& map, loamx_ctx* ctx, loamx_surfel_map* cmap, uint32_t min_points) {
  const std::vector<Surfel> got = map.surfels(min_points);
  const SurfelMapStats s = map.stats();
  loamx_surfel_map_stats cs;
  CHECK(loamx_surfel_map_stats_read(ctx, cmap, &cs) == LOAMX_OK);
  CHECK(s.voxels == cs.voxels && s.points_offered == cs.points_offered && s.points_used == cs.points_used && s.invalid == cs.invalid &&
        s.range == cs.range && s.outside == cs.outside && s.overflow == cs.overflow && s.overflow == 0);
  const size_t room = (size_t)cs.voxels + 1;
  std::vector<loamx_surfel> want(room);
  size_t n = 0;
  CHECK(loamx_surfel_map_emit_host(ctx, cmap, min_points, want.data(), room, &n) == LOAMX_OK);
  CHECK(n == got.size() && n <= cs.voxels);
  if (n != got.size()) return;
  CHECK(n == 0 || std::memcmp(want.data(), got.data(), n * sizeof(loamx_surfel)) == 0);
  for (size_t i = 0; i < n; i++) {
    const Surfel& r = got[i];
    const double len = r.normal[0] * r.normal[0] + r.normal[1] * r.normal[1] + r.normal[2] * r.normal[2];
    CHECK(r.count >= min_points && (i == 0 || r.first > got[i - 1].first) && std::fabs(len - 1.0) < 1e-12);
    CHECK(r.eval[0] <= r.eval[1] && r.eval[1] <= r.eval[2]);
  }
  // the query at the surfels' own means finds them again, at distance 0
  std::vector<double> xyz;
  for (const Surfel& r : got) xyz.insert(xyz.end(), r.mean, r.mean + 3);
  xyz.insert(xyz.end(), {1e3, 1e3, 1e3});  // no voxel there
  const SurfelQuery q = map.query(xyz, min_points);
  CHECK(q.size() == n + 1 && q.surfels.size() == n + 1 && q.distances.size() == n + 1);
  if (q.size() != n + 1) return;
  CHECK(n == 0 || std::memcmp(q.surfels.data(), got.data(), n * sizeof(Surfel)) == 0);
  for (size_t i = 0; i < n; i++) CHECK(q.counts[i] == got[i].count && q.distances[i] == 0.0);
  Surfel zero;
  std::memset(&zero, 0, sizeof(zero));
  CHECK(q.counts[n] == 0 && q.distances[n] == 0.0 && std::memcmp(&q.surfels[n], &zero, sizeof(zero)) == 0);
}

int main() {
  SurfelMapParams params;
  loamx_surfel_map_params cp;
  loamx_default_surfel_map_params(&cp);
  CHECK(params.leaf == 0.5 && params.min_range == 0.5 && params.max_range == 120.0);
  CHECK(cp.leaf == params.leaf && cp.min_range == params.min_range && cp.max_range == params.max_range);

  params.leaf = cp.leaf = 0.4;
  SurfelMap map(params, 1 << 14);
  loamx_ctx* ctx = gpu::defaultContext();
  loamx_surfel_map* cmap = nullptr;
  CHECK(loamx_surfel_map_create(ctx, &cp, 1 << 14, &cmap) == LOAMX_OK);
  CHECK(map.maxVoxels() == (1u << 14) && map.params().leaf == 0.4);
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
        CHECK(loamx_surfel_map_add_cloud_host(ctx, cmap, xyz.data(), 3, pts.size(), nullptr) == LOAMX_OK);
      } else {
        map.add(pts, pose);
        CHECK(loamx_surfel_map_add_cloud_host(ctx, cmap, xyz.data(), 3, pts.size(), back) == LOAMX_OK);
      }
      std::vector<PointF> ptsf;
      for (const PointD& p : scan(place, 1)) ptsf.push_back(PointF{(float)p.x, (float)p.y, (float)p.z, 1.0f});
      const std::vector<float> xyzf = gpu::packFloat(ptsf);
      map.add(ptsf, pose);
      CHECK(loamx_surfel_map_add_cloud_host_f32(ctx, cmap, xyzf.data(), 3, ptsf.size(), back) == LOAMX_OK);
    }
    compare(map, ctx, cmap, 1);
    compare(map, ctx, cmap, 3);
    const SurfelMapStats s = map.stats();
    CHECK(s.points_offered == 6u * 16u * 240u && s.voxels > 500 && s.points_used > s.voxels);
    CHECK(map.surfels(0xFFFFFFFFu).size() == 0);
    map.clear();
    CHECK(loamx_surfel_map_clear(ctx, cmap) == LOAMX_OK);
    CHECK(map.stats().voxels == 0 && map.stats().points_offered == 0 && map.surfels().size() == 0);
  }

  bool threw = false;
  try {
    SurfelMapParams bad;
    bad.leaf = 0.0;
    SurfelMap refused(bad);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);

  loamx_surfel_map_destroy(ctx, cmap);
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
