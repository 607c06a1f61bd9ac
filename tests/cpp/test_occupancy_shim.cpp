// test_occupancy_shim.cpp — loam::OccupancyMap (include/loam/occupancy.h) through the C++ headers: the counts and states of a
// query, a box and a slice and the stats are the C ABI's (loamx_occupancy_add_cloud[_f32] and the host read-outs on the same packed
// points and a map of its own), for double and float points, with and without a pose, before and after clear().
// Built and run by tests/test_gpu_occupancy_modules.py (needs a GPU).
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

// the header's map against the C ABI's, byte for byte; returns the number of occupied / free voxels of the box
static std::array<size_t, 2> compare(const OccupancyMap& map, loamx_ctx* ctx, loamx_occupancy_map* cmap, const std::vector<double>& probe) {
  const OccupancyStats s = map.stats();
  loamx_occupancy_stats cs;
  CHECK(loamx_occupancy_stats_read(ctx, cmap, &cs) == LOAMX_OK);
  CHECK(s.rays_offered == cs.rays_offered && s.rays_hit == cs.rays_hit && s.invalid == cs.invalid && s.range_short == cs.range_short &&
        s.range_long == cs.range_long && s.outside == cs.outside && s.visits == cs.visits && s.voxels == cs.voxels && s.overflow == cs.overflow &&
        s.overflow == 0);
  const std::array<int32_t, 3> vmin = {-40, -40, -6};
  const std::array<uint32_t, 3> dims = {80, 80, 12};
  const size_t n = (size_t)dims[0] * dims[1] * dims[2];
  const OccupancyCells box = map.box(vmin, dims);
  std::vector<uint32_t> counts(2 * n);
  std::vector<uint8_t> states(n);
  CHECK(loamx_occupancy_box(ctx, cmap, vmin.data(), dims.data(), counts.data(), states.data()) == LOAMX_OK);
  CHECK(box.size() == n && box.counts.size() == 2 * n);
  CHECK(std::memcmp(counts.data(), box.counts.data(), 2 * n * sizeof(uint32_t)) == 0 && std::memcmp(states.data(), box.states.data(), n) == 0);
  const std::vector<uint8_t> grid = map.slice(vmin, dims);
  std::vector<uint8_t> cgrid((size_t)dims[0] * dims[1]);
  CHECK(loamx_occupancy_slice(ctx, cmap, vmin.data(), dims.data(), cgrid.data()) == LOAMX_OK);
  CHECK(grid.size() == cgrid.size() && std::memcmp(grid.data(), cgrid.data(), grid.size()) == 0);
  const OccupancyCells q = map.query(probe);
  const size_t m = probe.size() / 3;
  std::vector<uint32_t> qcounts(2 * m);
  std::vector<uint8_t> qstates(m);
  CHECK(loamx_occupancy_query(ctx, cmap, probe.data(), 3, m, qcounts.data(), qstates.data()) == LOAMX_OK);
  CHECK(q.size() == m && (m == 0 || (std::memcmp(qcounts.data(), q.counts.data(), 2 * m * sizeof(uint32_t)) == 0 &&
                                     std::memcmp(qstates.data(), q.states.data(), m) == 0)));
  std::array<size_t, 2> seen = {0, 0};
  for (size_t i = 0; i < n; i++) {
    seen[0] += box.state(i) == Occupancy::OCCUPIED, seen[1] += box.state(i) == Occupancy::FREE;
    CHECK((box.state(i) == Occupancy::OCCUPIED) == (box.counts[2 * i] >= 1));  // (the default thresholds)
  }
  return seen;
}

int main() {
  OccupancyParams params;
  loamx_occupancy_params cp;
  loamx_default_occupancy_params(&cp);
  CHECK(params.leaf == 0.2 && params.min_range == 0.5 && params.max_range == 80.0 && params.end_margin == 0.2 && params.clip_long &&
        params.min_hits == 1 && params.occ_ratio == 0.0 && params.min_passes == 1);
  CHECK(cp.leaf == params.leaf && cp.min_range == params.min_range && cp.max_range == params.max_range && cp.end_margin == params.end_margin &&
        cp.clip_long == 1 && cp.min_hits == params.min_hits && cp.occ_ratio == params.occ_ratio && cp.min_passes == params.min_passes);

  params.leaf = cp.leaf = 0.5;
  params.max_range = cp.max_range = 30.0;
  OccupancyMap map(params, 1 << 17);
  loamx_ctx* ctx = gpu::defaultContext();
  loamx_occupancy_map* cmap = nullptr;
  CHECK(loamx_occupancy_create(ctx, &cp, 1 << 17, &cmap) == LOAMX_OK);
  CHECK(map.maxVoxels() == (1u << 17) && map.params().leaf == 0.5);
  const std::vector<double> probe = gpu::pack<FieldAccessor>(scan(0, 0));
  compare(map, ctx, cmap, probe);  // both empty

  for (int round = 0; round < 2; round++) {
    for (uint64_t place = 0; place < 3; place++) {
      const std::vector<PointD> pts = scan(place, 0);
      const std::vector<double> xyz = gpu::pack<FieldAccessor>(pts);
      double p7[7];
      loamx_synth_pair_pose(7, place, p7);
      const Pose3d pose = Pose3d::fromArray(p7);
      double back[7];
      pose.toArray(back);
      if (place == 0) {
        map.add(pts);  // the sensor at the map's origin
        CHECK(loamx_occupancy_add_cloud(ctx, cmap, xyz.data(), 3, pts.size(), nullptr) == LOAMX_OK);
      } else {
        map.add(pts, pose);
        CHECK(loamx_occupancy_add_cloud(ctx, cmap, xyz.data(), 3, pts.size(), back) == LOAMX_OK);
      }
      std::vector<PointF> ptsf;
      for (const PointD& p : scan(place, 1)) ptsf.push_back(PointF{(float)p.x, (float)p.y, (float)p.z, 1.0f});
      const std::vector<float> xyzf = gpu::packFloat(ptsf);
      map.add(ptsf, pose);
      CHECK(loamx_occupancy_add_cloud_f32(ctx, cmap, xyzf.data(), 3, ptsf.size(), back) == LOAMX_OK);
    }
    const std::array<size_t, 2> seen = compare(map, ctx, cmap, probe);
    const OccupancyStats s = map.stats();
    CHECK(s.rays_offered == 6u * 16u * 240u && s.rays_hit > 1000 && s.visits > 10 * s.rays_hit && s.voxels > 1000);
    CHECK(seen[0] > 100 && seen[1] > 1000);
    const OccupancyCells q = map.query(probe);  // the first cloud's own returns: every one that made a hit is in an occupied voxel
    size_t occupied = 0;
    for (size_t i = 0; i < q.size(); i++) occupied += q.state(i) == Occupancy::OCCUPIED;
    CHECK(occupied > q.size() / 2);
    map.clear();
    CHECK(loamx_occupancy_clear(ctx, cmap) == LOAMX_OK);
    CHECK(map.stats().voxels == 0 && map.stats().rays_offered == 0 && map.query(probe).state(0) == Occupancy::UNKNOWN);
  }

  bool threw = false;
  try {
    OccupancyParams bad;
    bad.leaf = 0.0;
    OccupancyMap refused(bad);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);

  loamx_occupancy_destroy(ctx, cmap);
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
