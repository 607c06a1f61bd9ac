// test_localize_shim.cpp — loam::SurfelMap::localize (include/loam/surfelmap.h) through the C++ headers: the pose, the result record
// and the information matrix are the C ABI's (loamx_surfel_localizer_run_host[_f32] on the same packed points, a map and a localiser of
// its own), for double and float points, at the defaults and at other parameters, and again after the map has grown.
// Built and run by tests/test_gpu_localize_modules.py (needs a GPU).
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

static loamx_localize_params toC(const LocalizeParams& q) {
  loamx_localize_params p;
  loamx_default_localize_params(&p);
  p.neighborhood = q.neighborhood, p.min_points = q.min_points, p.planarity = q.planarity, p.max_distance = q.max_distance;
  p.huber_delta = q.huber_delta, p.max_iterations = q.max_iterations, p.min_rows = q.min_rows;
  p.rotation_convergence_thresh = q.rotation_convergence_thresh, p.position_convergence_thresh = q.position_convergence_thresh;
  p.min_eigenvalue_per_row = q.min_eigenvalue_per_row;
  return p;
}

static void same(const Localization& got, const loamx_localize_result& res, const loamx_reg_information& info) {
  CHECK(std::memcmp(&got.result, &res, sizeof(res)) == 0);
  double pose[7];
  got.map_T_cloud.toArray(pose);
  const Pose3d want = Pose3d::fromArray(res.pose);
  double back[7];
  want.toArray(back);
  CHECK(std::memcmp(pose, back, sizeof(pose)) == 0);
  CHECK(std::memcmp(got.information.information, info.information, sizeof(info.information)) == 0);
  CHECK(std::memcmp(got.information.eigenvalues, info.eigenvalues, sizeof(info.eigenvalues)) == 0);
  CHECK(std::memcmp(got.information.eigenvectors, info.eigenvectors, sizeof(info.eigenvectors)) == 0);
  CHECK(std::memcmp(got.information.gradient, info.gradient, sizeof(info.gradient)) == 0);
  CHECK(got.information.weighted_sq_error == info.weighted_sq_error && got.information.n_plane == info.n_plane && got.information.n_edge == 0);
  CHECK(got.information.n_huber == info.n_huber && got.information.n_dropped == 0 && info.n_plane == res.n_rows);
  CHECK(got.converged() == (res.termination == LOAMX_LOCALIZE_CONVERGED));
}

int main() {
  LocalizeParams params;
  loamx_localize_params cp;
  loamx_default_localize_params(&cp);
  CHECK(params.neighborhood == cp.neighborhood && params.min_points == cp.min_points && params.planarity == cp.planarity);
  CHECK(params.max_distance == cp.max_distance && params.huber_delta == cp.huber_delta && params.max_iterations == cp.max_iterations);
  CHECK(params.min_rows == cp.min_rows && params.rotation_convergence_thresh == cp.rotation_convergence_thresh);
  CHECK(params.position_convergence_thresh == cp.position_convergence_thresh && params.min_eigenvalue_per_row == cp.min_eigenvalue_per_row);
  CHECK(cp.neighborhood == 7 && cp.min_points == 5 && cp.max_iterations == 10 && cp.min_rows == 100);

  SurfelMapParams mp;
  loamx_surfel_map_params cmp;
  loamx_default_surfel_map_params(&cmp);
  mp.leaf = cmp.leaf = 0.8;  // (sixteen scan lines in a room: smaller voxels hold lines, not planes)
  SurfelMap map(mp, 1 << 14);
  loamx_ctx* ctx = gpu::defaultContext();
  loamx_surfel_map* cmap = nullptr;
  CHECK(loamx_surfel_map_create(ctx, &cmp, 1 << 14, &cmap) == LOAMX_OK);
  loamx_surfel_localizer* cloc = nullptr;
  CHECK(loamx_surfel_localizer_create(ctx, cmap, 1, 16 * 240, &cloc) == LOAMX_OK);

  const std::vector<PointD> pts = scan(0, 0);
  const std::vector<double> xyz = gpu::pack<FieldAccessor>(pts);
  std::vector<PointF> ptsf;
  for (const PointD& p : pts) ptsf.push_back(PointF{(float)p.x, (float)p.y, (float)p.z, 1.0f});
  const std::vector<float> xyzf = gpu::packFloat(ptsf);
  // a small motion away from where the scan was taken
  const double half = 0.004;
  const double start7[7] = {0.0, 0.0, std::sin(half), std::cos(half), 0.05, -0.04, 0.02};
  const Pose3d start = Pose3d::fromArray(start7);
  double start_back[7];
  start.toArray(start_back);

  for (int round = 0; round < 2; round++) {
    // round 0: the scan itself is the map; round 1: a second scan of the same place has been added
    const std::vector<PointD> more = scan(0, round == 0 ? 0 : 1);
    const std::vector<double> more_xyz = gpu::pack<FieldAccessor>(more);
    if (round == 0) {
      map.add(more);
      CHECK(loamx_surfel_map_add_cloud_host(ctx, cmap, more_xyz.data(), 3, more.size(), nullptr) == LOAMX_OK);
    } else {
      double p7[7];
      loamx_synth_pair_pose(7, 0, p7);
      const Pose3d pose = Pose3d::fromArray(p7);
      double back[7];
      pose.toArray(back);
      map.add(more, pose);
      CHECK(loamx_surfel_map_add_cloud_host(ctx, cmap, more_xyz.data(), 3, more.size(), back) == LOAMX_OK);
    }
    for (int variant = 0; variant < 3; variant++) {
      LocalizeParams q;
      if (variant == 1) q.neighborhood = 1, q.max_iterations = 3, q.huber_delta = 0.0;
      if (variant == 2) q.max_iterations = 0;
      const loamx_localize_params cq = toC(q);
      loamx_localize_result res;
      loamx_reg_information info;
      const Localization got = map.localize(pts, start, q);
      CHECK(loamx_surfel_localizer_run_host(ctx, cloc, xyz.data(), 3, pts.size(), start_back, &cq, &res, &info) == LOAMX_OK);
      same(got, res, info);
      CHECK(res.n_rows > 500);
      if (variant == 0 && round == 0) {
        CHECK(res.termination == LOAMX_LOCALIZE_CONVERGED && res.iterations >= 1 && res.final_cost < res.initial_cost);
        CHECK(std::fabs(res.pose[4]) < 0.02 && std::fabs(res.pose[5]) < 0.02 && std::fabs(res.pose[6]) < 0.02);  // back where the scan was taken
      }
      if (variant == 2) CHECK(res.iterations == 0 && std::memcmp(res.pose, start_back, sizeof(start_back)) == 0);
      const Localization gotf = map.localize(ptsf, start, q);
      CHECK(loamx_surfel_localizer_run_host_f32(ctx, cloc, xyzf.data(), 3, ptsf.size(), start_back, &cq, &res, &info) == LOAMX_OK);
      same(gotf, res, info);
    }
  }

  bool threw = false;
  try {
    LocalizeParams bad;
    bad.neighborhood = 3;
    map.localize(pts, start, bad);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);

  loamx_surfel_localizer_destroy(ctx, cloc);
  loamx_surfel_map_destroy(ctx, cmap);
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
