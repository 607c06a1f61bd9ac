// test_organize_shim.cpp — loam::organizeCloud (include/loam/organize.h) through the C++ headers: the index map and the counters
// are the C ABI's (loamx_organize_cloud[_f32] on the same packed points), for double and float points, with and without ring
// numbers; the scan holds the winners copied whole (the intensity comes along) and the given point in the empty cells.
// Built and run by tests/test_gpu_organize_modules.py (needs a GPU).
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

// a 16 x 256 synthetic scan with its points dealt out of order (a fixed stride walk) and the line of every point as its ring
template <typename P, typename Make>
static void shuffled(std::vector<P>& cloud, std::vector<uint16_t>& rings, Make make) {
  const uint32_t H = 16, W = 256, n = H * W;
  std::vector<double> xyz(n * 3);
  loamx_synth_scan_host(3, 2, 0, H, W, 0.01, xyz.data());
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t j = (uint32_t)(((uint64_t)i * 2654435761ull + 12345u) % n);  // (odd multiplier, n a power of two: a permutation)
    cloud.push_back(make(xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2], (int)j));
    rings.push_back((uint16_t)(j / W));
  }
}

template <typename P, typename T, typename Pack, typename CFn>
static void compare(const std::vector<P>& cloud, const std::vector<uint16_t>& rings, const ScanLayout& layout, const P& empty, Pack pack, CFn cfn) {
  const std::vector<T> xyz = pack(cloud);
  for (int with_rings = 0; with_rings < 2; with_rings++) {
    const std::vector<uint16_t> r = with_rings ? rings : std::vector<uint16_t>();
    const OrganizedCloud<P> got = organizeCloud(cloud, layout, r, empty);
    std::vector<T> scan(layout.cells() * 3);
    std::vector<uint32_t> src(layout.cells());
    uint32_t st[4];
    CHECK(cfn(gpu::defaultContext(), layout.handle(), xyz.data(), 3, with_rings ? rings.data() : nullptr, cloud.size(), scan.data(), src.data(), st) ==
          LOAMX_OK);
    CHECK(got.src_idx == src);
    CHECK(got.filled == st[0] && got.invalid == st[1] && got.outside == st[2] && got.collisions == st[3]);
    CHECK((size_t)st[0] + st[1] + st[2] + st[3] == cloud.size() && st[0] > cloud.size() / 2);
    CHECK(got.scan.size() == layout.cells());
    size_t wrong = 0;
    for (size_t c = 0; c < layout.cells(); c++) {
      const P& p = got.scan[c];
      const T want[3] = {scan[3 * c], scan[3 * c + 1], scan[3 * c + 2]};
      const T have[3] = {(T)p.x, (T)p.y, (T)p.z};
      if (std::memcmp(want, have, sizeof(want)) != 0) wrong++;
      if (src[c] != OrganizedCloud<P>::kNoPoint && !same_point(p, cloud[src[c]])) wrong++;
      if (src[c] == OrganizedCloud<P>::kNoPoint && !same_point(p, empty)) wrong++;
    }
    CHECK(wrong == 0);
    if (with_rings) CHECK(st[2] == 0);  // every ring names a line
  }
}

int main() {
  const LidarParams lidar(16, 256, 1.0, 120.0);
  OrganizeParams params;
  params.fov_bottom = -0.45, params.fov_top = 0.3;
  const ScanLayout first(lidar, params);
  params.keep = OrganizeKeep::Nearest;
  const ScanLayout nearest(lidar, params);
  CHECK(first.columnDirections().size() == 512 && first.lineTangents().size() == 17 && first.cells() == 4096);
  CHECK(first.lineTangents()[0] < first.lineTangents()[16]);

  std::vector<PointD> cd;
  std::vector<PointF> cf;
  std::vector<uint16_t> rd, rf;
  shuffled(cd, rd, [](double x, double y, double z, int tag) { return PointD(x, y, z, tag); });
  shuffled(cf, rf, [](double x, double y, double z, int tag) {
    PointF p;
    p.x = (float)x, p.y = (float)y, p.z = (float)z, p.intensity = (float)tag;
    return p;
  });
  for (const ScanLayout* layout : {&first, &nearest}) {
    compare<PointD, double>(cd, rd, *layout, PointD(0, 0, 0, -7), [](const std::vector<PointD>& c) { return gpu::pack<FieldAccessor>(c); },
                            loamx_organize_cloud);
    compare<PointF, float>(cf, rf, *layout, PointF(), [](const std::vector<PointF>& c) { return gpu::packFloat(c); }, loamx_organize_cloud_f32);
  }
  // the default empty point, and what goes on from here: the organised scan is a scan for extractFeatures
  const OrganizedCloud<PointF> scan = organizeCloud(cf, first);
  CHECK(scan.scan.size() == 4096);
  const LoamFeatures<PointF> feats = extractFeatures(scan.scan, lidar);
  CHECK(feats.planar_points.size() > 100);
  // refusals arrive as exceptions
  bool threw = false;
  try {
    organizeCloud(cf, first, std::vector<uint16_t>(5, 0));
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);
  threw = false;
  try {
    OrganizeParams bad;
    bad.elevations = {0.1, 0.0};
    ScanLayout l(LidarParams(2, 8, 1.0, 120.0), bad);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
