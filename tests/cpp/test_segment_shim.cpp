// test_segment_shim.cpp — loam::segmentScan (include/loam/segment.h) through the C++ headers: classes, labels, sizes, the
// accepted components and the counters are the C ABI's (loamx_segment_scan[_f32] on the same packed scan), for double and
// float points; a kept cell of the filtered scan is the input point copied whole (the tag comes along) and reads as the C ABI's
// filtered cell, a dropped one is the given point. Built and run by tests/test_gpu_segment_modules.py (needs a GPU).
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
  int tag;
  PointD(double x, double y, double z, int tag) : x(x), y(y), z(z), tag(tag) {}
};
struct PointF {
  float x = 0, y = 0, z = 0, intensity = -1.0f;
};
static bool same_point(const PointD& a, const PointD& b) { return std::memcmp(&a.x, &b.x, 3 * sizeof(double)) == 0 && a.tag == b.tag; }
static bool same_point(const PointF& a, const PointF& b) { return std::memcmp(&a.x, &b.x, 4 * sizeof(float)) == 0; }

// walls at 10 m and 20 m in blocks, holes, a floor under the lower lines, a few stray returns: every class occurs
static std::vector<double> scene(uint32_t H, uint32_t W) {
  std::vector<double> xyz(3 * (size_t)H * W);
  uint64_t s = 0x9E3779B97F4A7C15ull;
  for (uint32_t l = 0; l < H; l++)
    for (uint32_t c = 0; c < W; c++) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      const double u = (double)(s >> 11) / 9007199254740992.0;
      const double az = 2.0 * M_PI * c / W, el = (-24.0 + 2.0 * l) * M_PI / 180.0;
      double r = ((c / 24) % 2) ? 10.0 : 20.0;
      if (el < -0.1) r = 1.8 / -std::sin(el);
      if (u < 0.05) r = 0.0;
      else if (u < 0.10) r = 5.0 + 3.0 * u;
      double* p = &xyz[3 * ((size_t)l * W + c)];
      p[0] = r * std::cos(el) * std::cos(az), p[1] = r * std::cos(el) * std::sin(az), p[2] = r * std::sin(el);
    }
  return xyz;
}

template <typename P, typename T, typename CFn>
static void compare(const std::vector<P>& scan, const std::vector<T>& xyz, const LidarParams& lidar, const SegmentationParams& params, const P& empty,
                    CFn cfn) {
  const size_t n = scan.size();
  const ScanSegmentation<P> got = segmentScan(scan, lidar, params, empty);
  const loamx_lidar_params lp = gpu::toC(lidar);
  const loamx_segment_params sp = gpu::toC(params);
  std::vector<uint8_t> classes(n);
  std::vector<uint32_t> labels(n), sizes(n);
  std::vector<T> filtered(3 * n);
  std::vector<loamx_segment_cluster> recs(n);
  uint32_t st[8];
  CHECK(cfn(gpu::defaultContext(), xyz.data(), &lp, &sp, classes.data(), labels.data(), sizes.data(), filtered.data(), recs.data(), n, st) == LOAMX_OK);
  CHECK(got.labels == labels && got.sizes == sizes);
  CHECK(got.classes.size() == n && got.filtered.size() == n);
  CHECK(got.invalid == st[0] && got.ground == st[1] && got.cluster_cells == st[2] && got.outlier_cells == st[3]);
  CHECK(got.accepted == st[4] && got.rejected == st[5] && got.largest == st[6] && got.clusters.size() == st[7] && st[7] == st[4]);
  CHECK((size_t)st[0] + st[1] + st[2] + st[3] == n && st[0] > 0 && st[1] > 0 && st[2] > 0 && st[3] > 0);
  CHECK(std::memcmp(got.clusters.data(), recs.data(), got.clusters.size() * sizeof(loamx_segment_cluster)) == 0);
  size_t wrong = 0;
  for (size_t i = 0; i < n; i++) {
    if ((uint8_t)got.classes[i] != classes[i]) wrong++;
    const P& p = got.filtered[i];
    const T want[3] = {filtered[3 * i], filtered[3 * i + 1], filtered[3 * i + 2]};
    const T have[3] = {(T)p.x, (T)p.y, (T)p.z};
    if (std::memcmp(want, have, sizeof(want)) != 0) wrong++;
    const bool kept = classes[i] == LOAMX_SEGMENT_CLUSTER || (classes[i] == LOAMX_SEGMENT_OUTLIER && !params.drop_outliers) ||
                      (classes[i] == LOAMX_SEGMENT_GROUND && !params.drop_ground);
    if (!same_point(p, kept ? scan[i] : empty)) wrong++;
  }
  CHECK(wrong == 0);
}

int main() {
  const uint32_t H = 21, W = 300;
  const LidarParams lidar(H, W, 1.0, 120.0);
  const std::vector<double> xyz = scene(H, W);
  std::vector<PointD> sd;
  std::vector<PointF> sf;
  std::vector<float> xyzf(xyz.size());
  for (size_t i = 0; i < (size_t)H * W; i++) {
    sd.push_back(PointD(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], (int)i));
    PointF p;
    p.x = (float)xyz[3 * i], p.y = (float)xyz[3 * i + 1], p.z = (float)xyz[3 * i + 2], p.intensity = (float)i;
    sf.push_back(p);
    xyzf[3 * i] = p.x, xyzf[3 * i + 1] = p.y, xyzf[3 * i + 2] = p.z;
  }
  SegmentationParams defaults, other;
  other.ground_lines = 9, other.drop_outliers = false, other.drop_ground = true, other.min_cluster_points = 12, other.segment_angle = 0.7;
  CHECK(defaults.ground_lines == 0 && defaults.min_cluster_points == 30 && defaults.min_tall_cluster_points == 5 && defaults.min_tall_cluster_lines == 3);
  loamx_segment_params c_defaults;
  loamx_default_segment_params(&c_defaults);
  CHECK(defaults.ground_angle == c_defaults.ground_angle && defaults.segment_angle == c_defaults.segment_angle && defaults.drop_outliers &&
        !defaults.drop_ground && c_defaults.drop_outliers == 1 && c_defaults.drop_ground == 0);
  for (const SegmentationParams* p : {&defaults, &other}) {
    compare<PointD, double>(sd, xyz, lidar, *p, PointD(0, 0, 0, -7), loamx_segment_scan);
    compare<PointF, float>(sf, xyzf, lidar, *p, PointF(), loamx_segment_scan_f32);
  }
  // the default empty point, and what goes on from here: the filtered scan is a scan for extractFeatures
  const ScanSegmentation<PointF> seg = segmentScan(sf, lidar);
  CHECK(seg.filtered.size() == (size_t)H * W && seg.accepted > 0);
  const LoamFeatures<PointF> feats = extractFeatures(seg.filtered, lidar);
  CHECK(feats.planar_points.size() > 50);
  // refusals arrive as exceptions
  bool threw = false;
  try {
    segmentScan(std::vector<PointF>(5), lidar);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);
  threw = false;
  try {
    SegmentationParams bad;
    bad.segment_angle = 2.0;
    segmentScan(sf, lidar, bad);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
