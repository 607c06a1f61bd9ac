// test_raycast_shim.cpp — loam::OccupancyMap::castRays / renderScans (include/loam/occupancy.h) through the C++ headers: the records,
// points and ranges are the C ABI's (loamx_occupancy_cast_rays_host / _render_scans_host on a map of its own that took the same
// clouds). The C ABI's bytes are compared with the Python model by tests/test_gpu_raycast.py. Built and run by
// tests/test_gpu_raycast_modules.py (needs a GPU).
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

int main() {
  RaycastParams rp;
  loamx_raycast_params crp;
  loamx_default_raycast_params(&crp);
  CHECK(rp.skip_start == crp.skip_start && rp.max_steps == crp.max_steps && rp.max_steps == 3 * 4098 && (uint32_t)rp.hit_at == crp.hit_at);
  CHECK(!rp.unknown_stops && crp.unknown_stops == 0 && rp.hit_at == RaycastParams::AT_MIDDLE);
  CHECK(sizeof(RayRecord) == 40 && RayRecord::HIT == 1 && RayRecord::INVALID == 5);

  OccupancyParams params;
  loamx_occupancy_params cp;
  loamx_default_occupancy_params(&cp);
  params.leaf = cp.leaf = 0.5;
  params.max_range = cp.max_range = 30.0;
  params.end_margin = cp.end_margin = 0.0;
  OccupancyMap map(params, 1 << 17);
  loamx_ctx* ctx = gpu::defaultContext();
  loamx_occupancy_map* cmap = nullptr;
  CHECK(loamx_occupancy_create(ctx, &cp, 1 << 17, &cmap) == LOAMX_OK);

  const std::vector<PointD> pts = scan(0, 0);
  const std::vector<double> xyz = gpu::pack<FieldAccessor>(pts);
  double p7[7], back[7];
  loamx_synth_pair_pose(7, 0, p7);
  const Pose3d pose = Pose3d::fromArray(p7);
  pose.toArray(back);
  map.add(pts, pose);
  CHECK(loamx_occupancy_add_cloud(ctx, cmap, xyz.data(), 3, pts.size(), back) == LOAMX_OK);

  // segments from the sensor to every 7th return, stretched by a fifth: most of them meet the voxel of their return
  std::vector<double> origins, ends;
  for (size_t i = 0; i < pts.size(); i += 7) {
    const Vector3d e = pose.act(Vector3d(1.2 * pts[i].x, 1.2 * pts[i].y, 1.2 * pts[i].z));
    for (int a = 0; a < 3; a++) origins.push_back(back[4 + a]), ends.push_back(e[a]);
  }
  const size_t n = origins.size() / 3;
  for (int variant = 0; variant < 3; variant++) {
    rp = RaycastParams();
    if (variant == 1) rp.unknown_stops = true, rp.skip_start = 1;
    if (variant == 2) rp.max_steps = 6;
    crp.skip_start = rp.skip_start, crp.unknown_stops = rp.unknown_stops ? 1u : 0u, crp.max_steps = rp.max_steps, crp.hit_at = rp.hit_at;
    const std::vector<RayRecord> got = map.castRays(origins, ends, rp);
    std::vector<loamx_ray_record> want(n);
    CHECK(loamx_occupancy_cast_rays_host(ctx, cmap, origins.data(), ends.data(), 3, n, &crp, want.data()) == LOAMX_OK);
    CHECK(got.size() == n && std::memcmp(got.data(), want.data(), n * sizeof(loamx_ray_record)) == 0);
    size_t hits = 0, truncated = 0;
    for (const RayRecord& r : got) hits += r.hit(), truncated += r.status == RayRecord::TRUNCATED;
    CHECK(variant == 2 ? truncated > n / 2 : hits > n / 2);
  }

  // the scan the map predicts at the pose it was filled from, for a fan of beams
  std::vector<double> dirs;
  for (int l = 0; l < 4; l++)
    for (int c = 0; c < 70; c++) {
      const double el = -0.2 + 0.1 * l, az = 6.283185307179586 * c / 70.0;
      dirs.insert(dirs.end(), {std::cos(el) * std::cos(az), std::cos(el) * std::sin(az), std::sin(el)});
    }
  for (int at = 0; at < 2; at++) {
    rp = RaycastParams();
    rp.hit_at = at ? RaycastParams::AT_MIDDLE : RaycastParams::AT_ENTER;
    crp.skip_start = 0, crp.unknown_stops = 0, crp.max_steps = rp.max_steps, crp.hit_at = rp.hit_at;
    const RenderedScans r = map.renderScans(dirs, {pose, Pose3d()}, 25.0, rp);
    const size_t m = 2 * 280;
    std::vector<double> poses(back, back + 7), sc(3 * m), rg(m);
    double ident[7];
    Pose3d().toArray(ident);
    poses.insert(poses.end(), ident, ident + 7);
    std::vector<loamx_ray_record> rec(m);
    CHECK(loamx_occupancy_render_scans_host(ctx, cmap, dirs.data(), 280, poses.data(), 2, 25.0, &crp, sc.data(), rg.data(), rec.data()) == LOAMX_OK);
    CHECK(r.n_poses == 2 && r.n_beams == 280 && r.xyz.size() == 3 * m && r.ranges.size() == m && r.records.size() == m);
    CHECK(std::memcmp(r.xyz.data(), sc.data(), 3 * m * sizeof(double)) == 0 && std::memcmp(r.ranges.data(), rg.data(), m * sizeof(double)) == 0);
    CHECK(std::memcmp(r.records.data(), rec.data(), m * sizeof(loamx_ray_record)) == 0);
    size_t hits = 0;
    bool consistent = true;
    for (size_t i = 0; i < m; i++) {
      hits += r.records[i].hit();
      if (!r.records[i].hit()) consistent = consistent && r.ranges[i] == 0.0 && r.xyz[3 * i] == 0.0 && r.xyz[3 * i + 1] == 0.0 && r.xyz[3 * i + 2] == 0.0;
      else consistent = consistent && r.ranges[i] <= 25.0 && r.xyz[3 * i + 2] == r.ranges[i] * dirs[3 * (i % 280) + 2];
    }
    CHECK(consistent && hits > 50);
  }

  bool threw = false;
  try {
    rp = RaycastParams();
    rp.max_steps = (1u << 22) + 1u;
    map.castRays(origins, ends, rp);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);
  threw = false;
  try {
    map.renderScans(dirs, {pose}, -1.0);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);

  loamx_occupancy_destroy(ctx, cmap);
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
