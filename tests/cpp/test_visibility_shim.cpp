// test_visibility_shim.cpp — loam::visibilityVotes / loam::removeDynamicPoints (include/loam/visibility.h) through the C++ headers:
// the votes are the C ABI's (loamx_visibility_votes[_f32] on the same packed points, scans and poses), the flags, the kept indices
// and the kept points are loamx_visibility_filter_dev's, for double and float scans.
// Built and run by tests/test_gpu_visibility_modules.py (needs a GPU).
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

static const uint32_t H = 16, W = 240;

static std::vector<PointD> scan(uint64_t pair, uint32_t which) {
  const uint32_t n = H * W;
  std::vector<double> xyz(n * 3);
  loamx_synth_scan_host(7, pair, which, H, W, 0.01, xyz.data());
  std::vector<PointD> out;
  for (uint32_t i = 0; i < n; i++) out.push_back(PointD{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]});
  return out;
}

// the header's cleaned map against loamx_visibility_filter_dev on buffers of this test's own
static void compare_filter(const std::vector<PointD>& map_points, const std::vector<VisibilityVotes>& votes, const VisibilityParams& params) {
  const auto got = removeDynamicPoints(map_points, votes, params);
  loamx_ctx* ctx = gpu::defaultContext();
  const loamx_visibility_params vp = gpu::toC(params);
  const size_t n = votes.size();
  const std::vector<double> xyz = gpu::pack<FieldAccessor>(map_points);
  void *d_votes = nullptr, *d_pts = nullptr, *d_dyn = nullptr, *d_xyz = nullptr, *d_idx = nullptr, *d_n = nullptr;
  CHECK(loamx_dev_alloc(ctx, n * 16 + 16, &d_votes) == LOAMX_OK && loamx_dev_alloc(ctx, n * 24 + 16, &d_pts) == LOAMX_OK);
  CHECK(loamx_dev_alloc(ctx, n + 16, &d_dyn) == LOAMX_OK && loamx_dev_alloc(ctx, n * 24 + 16, &d_xyz) == LOAMX_OK);
  CHECK(loamx_dev_alloc(ctx, n * 4 + 16, &d_idx) == LOAMX_OK && loamx_dev_alloc(ctx, 4, &d_n) == LOAMX_OK);
  if (n) CHECK(loamx_copy_to_device(ctx, d_votes, votes.data(), n * 16) == LOAMX_OK && loamx_copy_to_device(ctx, d_pts, xyz.data(), n * 24) == LOAMX_OK);
  CHECK(loamx_visibility_filter_dev(ctx, static_cast<loamx_visibility_tally*>(d_votes), n, &vp, static_cast<double*>(d_pts), 3, static_cast<uint8_t*>(d_dyn),
                                    static_cast<double*>(d_xyz), static_cast<uint32_t*>(d_idx), n, static_cast<uint32_t*>(d_n)) == LOAMX_OK);
  uint32_t kept = 0;
  CHECK(loamx_copy_to_host(ctx, &kept, d_n, 4) == LOAMX_OK);
  std::vector<uint8_t> dyn(n);
  std::vector<uint32_t> idx(kept);
  std::vector<double> out(3 * (size_t)kept);
  if (n) CHECK(loamx_copy_to_host(ctx, dyn.data(), d_dyn, n) == LOAMX_OK);
  if (kept) CHECK(loamx_copy_to_host(ctx, idx.data(), d_idx, kept * 4) == LOAMX_OK && loamx_copy_to_host(ctx, out.data(), d_xyz, kept * 24) == LOAMX_OK);
  CHECK(got.dynamic == dyn && got.static_index == idx && got.static_points.size() == kept);
  size_t n_dyn = 0;
  for (uint8_t d : dyn) n_dyn += d;
  CHECK(n_dyn + kept == n);
  if (got.static_points.size() == kept)
    for (size_t i = 0; i < kept; i++)
      CHECK(got.static_points[i].x == out[3 * i] && got.static_points[i].y == out[3 * i + 1] && got.static_points[i].z == out[3 * i + 2]);
  for (void* p : {d_votes, d_pts, d_dyn, d_xyz, d_idx, d_n}) loamx_dev_free(ctx, p);
}

int main() {
  VisibilityParams params;
  loamx_visibility_params cp;
  loamx_default_visibility_params(&cp);
  CHECK(params.min_range == 1.0 && params.max_range == 80.0 && params.margin == 0.3 && params.margin_rel == 0.01 && params.window_lines == 1 &&
        params.window_cols == 1 && params.min_through == 2 && params.through_ratio == 1.0);
  CHECK(cp.min_range == params.min_range && cp.max_range == params.max_range && cp.margin == params.margin && cp.margin_rel == params.margin_rel &&
        cp.window_lines == params.window_lines && cp.window_cols == params.window_cols && cp.min_through == params.min_through &&
        cp.through_ratio == params.through_ratio);
  static_assert(sizeof(VisibilityVotes) == 16, "four words");

  const LidarParams lidar(H, W, 1.0, 120.0);
  OrganizeParams op;  // the generator's fan: linear in [-22.5, 22.5] degrees
  op.fov_bottom = -22.5 * M_PI / 180.0, op.fov_top = 22.5 * M_PI / 180.0;
  ScanLayout layout(lidar, op);
  loamx_ctx* ctx = gpu::defaultContext();

  // three scans: a place, the same place a step on (at the pair's pose), and another place put where it is not
  std::vector<std::vector<PointD>> scans = {scan(0, 0), scan(0, 1), scan(1, 0)};
  double p7[7];
  loamx_synth_pair_pose(7, 0, p7);
  std::vector<Pose3d> poses = {Pose3d::Identity(), Pose3d::fromArray(p7), Pose3d::Identity()};
  std::vector<PointD> map_points;
  for (size_t s = 0; s < 2; s++)
    for (const PointD& p : scans[s]) {
      const Vector3d w = poses[s].act(Vector3d(p.x, p.y, p.z));
      if (p.x != 0.0 || p.y != 0.0 || p.z != 0.0) map_points.push_back(PointD{w(0), w(1), w(2)});
    }
  CHECK(map_points.size() > 1000);

  std::vector<double> pose_rows(7 * poses.size());
  for (size_t i = 0; i < poses.size(); i++) poses[i].toArray(pose_rows.data() + 7 * i);
  const std::vector<double> m = gpu::pack<FieldAccessor>(map_points);
  for (uint32_t window = 0; window < 2; window++) {
    params.window_lines = params.window_cols = cp.window_lines = cp.window_cols = window;
    // double scans
    const std::vector<VisibilityVotes> got = visibilityVotes(map_points, scans, poses, layout, params);
    std::vector<double> xyz;
    for (const auto& s : scans) {
      const std::vector<double> one = gpu::pack<FieldAccessor>(s);
      xyz.insert(xyz.end(), one.begin(), one.end());
    }
    std::vector<loamx_visibility_tally> want(map_points.size());
    CHECK(loamx_visibility_votes(ctx, layout.handle(), m.data(), 3, map_points.size(), xyz.data(), scans.size(), pose_rows.data(), &cp, want.data()) == LOAMX_OK);
    CHECK(got.size() == want.size() && std::memcmp(got.data(), want.data(), want.size() * sizeof(loamx_visibility_tally)) == 0);
    unsigned long long sums[4] = {0, 0, 0, 0};
    for (const auto& v : got) sums[0] += v.through, sums[1] += v.agree, sums[2] += v.occluded, sums[3] += v.empty;
    CHECK(sums[1] > map_points.size() / 2 && sums[0] + sums[2] > 0);
    // float scans
    std::vector<std::vector<PointF>> scansf;
    std::vector<float> xyzf;
    for (const auto& s : scans) {
      scansf.emplace_back();
      for (const PointD& p : s) scansf.back().push_back(PointF{(float)p.x, (float)p.y, (float)p.z, 1.0f});
      const std::vector<float> one = gpu::packFloat(scansf.back());
      xyzf.insert(xyzf.end(), one.begin(), one.end());
    }
    const std::vector<VisibilityVotes> gotf = visibilityVotes(map_points, scansf, poses, layout, params);
    CHECK(loamx_visibility_votes_f32(ctx, layout.handle(), m.data(), 3, map_points.size(), xyzf.data(), scans.size(), pose_rows.data(), &cp, want.data()) ==
          LOAMX_OK);
    CHECK(gotf.size() == want.size() && std::memcmp(gotf.data(), want.data(), want.size() * sizeof(loamx_visibility_tally)) == 0);

    compare_filter(map_points, got, params);
    VisibilityParams eager = params;
    eager.min_through = 1, eager.through_ratio = 0.5;
    compare_filter(map_points, got, eager);
  }
  compare_filter({}, {}, params);
  CHECK(visibilityVotes(std::vector<PointD>(), scans, poses, layout).empty());

  int threw = 0;
  try {
    VisibilityParams bad;
    bad.window_cols = 4;
    visibilityVotes(map_points, scans, poses, layout, bad);
  } catch (const std::runtime_error&) {
    threw++;
  }
  try {
    visibilityVotes(map_points, scans, std::vector<Pose3d>(2), layout);
  } catch (const std::runtime_error&) {
    threw++;
  }
  try {
    removeDynamicPoints(map_points, std::vector<VisibilityVotes>(3));
  } catch (const std::runtime_error&) {
    threw++;
  }
  CHECK(threw == 3);

  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
