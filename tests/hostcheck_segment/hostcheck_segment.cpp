// TEST-ONLY host build of loam_amd/csrc/segment_math.h: the validity, ground-pair and edge predicates of the segmentation
// kernels compiled with g++ (-ffp-contract=off), and a serial union-find over the same predicates, for
// tests/test_segment_hostcheck.py (compared with the numpy model of tests/segment_common.py by equality). With
// -DHOSTCHECK_SEGMENT_MAIN: a stand-alone program for `make san`.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../loam_amd/csrc/segment_math.h"

using namespace loamx;

namespace {

uint32_t find_root(std::vector<uint32_t>& parent, uint32_t x) {
  while (parent[x] != x) x = parent[x] = parent[parent[x]];
  return x;
}
void unite(std::vector<uint32_t>& parent, uint32_t a, uint32_t b) {
  a = find_root(parent, a), b = find_root(parent, b);
  if (a == b) return;
  if (a < b) parent[b] = a;  // only the minimum wins: the root is the component's smallest index
  else parent[a] = b;
}

}  // namespace

extern "C" {

void hostcheck_segment_valid(const double* p, uint64_t n, double min_range, double max_range, uint8_t* out) {
  for (uint64_t i = 0; i < n; i++) out[i] = seg_valid(p[3 * i], p[3 * i + 1], p[3 * i + 2], min_range, max_range) ? 1 : 0;
}

void hostcheck_segment_ground_pair(const double* a, const double* b, uint64_t n, double tg2, uint8_t* out) {
  for (uint64_t i = 0; i < n; i++)
    out[i] = seg_ground_pair(a[3 * i], a[3 * i + 1], a[3 * i + 2], b[3 * i], b[3 * i + 1], b[3 * i + 2], tg2) ? 1 : 0;
}

void hostcheck_segment_connected(const double* a, const double* b, uint64_t n, double c2, uint8_t* out) {
  for (uint64_t i = 0; i < n; i++)
    out[i] = seg_connected(a[3 * i], a[3 * i + 1], a[3 * i + 2], b[3 * i], b[3 * i + 1], b[3 * i + 2], c2) ? 1 : 0;
}

// one scan, serially: classes, labels, sizes and line spans (0 outside the components) per cell
void hostcheck_segment_scan(const double* p, uint32_t H, uint32_t W, uint32_t ground_lines, double min_range, double max_range, double tg2,
                            double c2, uint32_t min_cluster, uint32_t min_tall_points, uint32_t min_tall_lines, uint8_t* classes,
                            uint32_t* labels, uint32_t* sizes, uint32_t* spans) {
  SegParams P{};
  P.H = H, P.W = W, P.G = ground_lines == 0 || ground_lines > H ? H : ground_lines;
  P.min_range = min_range, P.max_range = max_range, P.tg2 = tg2, P.c2 = c2;
  P.min_cluster = min_cluster, P.min_tall_points = min_tall_points, P.min_tall_lines = min_tall_lines;
  const uint32_t HW = H * W;
  auto at = [&](uint32_t i, int k) { return p[3 * (size_t)i + k]; };
  auto valid = [&](uint32_t i) { return seg_valid(at(i, 0), at(i, 1), at(i, 2), min_range, max_range); };
  std::vector<uint8_t> cls(HW, kSegInvalid);
  for (uint32_t i = 0; i < HW; i++)
    if (valid(i)) cls[i] = kSegNode;
  std::vector<uint8_t> ground(HW, 0);
  for (uint32_t l = 0; l + 1 < P.G; l++)
    for (uint32_t c = 0; c < W; c++) {
      const uint32_t a = l * W + c, b = a + W;
      if (cls[a] != kSegInvalid && cls[b] != kSegInvalid && seg_ground_pair(at(a, 0), at(a, 1), at(a, 2), at(b, 0), at(b, 1), at(b, 2), tg2))
        ground[a] = ground[b] = 1;
    }
  for (uint32_t i = 0; i < HW; i++)
    if (ground[i]) cls[i] = kSegGround;
  std::vector<uint32_t> parent(HW);
  for (uint32_t i = 0; i < HW; i++) parent[i] = i;
  auto conn = [&](uint32_t a, uint32_t b) {
    return cls[a] == kSegNode && cls[b] == kSegNode && seg_connected(at(a, 0), at(a, 1), at(a, 2), at(b, 0), at(b, 1), at(b, 2), c2);
  };
  for (uint32_t l = 0; l < H; l++)
    for (uint32_t c = 0; c < W; c++) {
      const uint32_t i = l * W + c;
      if (W > 1 && conn(i, l * W + (c + 1 == W ? 0 : c + 1))) unite(parent, i, l * W + (c + 1 == W ? 0 : c + 1));
      if (l + 1 < H && conn(i, i + W)) unite(parent, i, i + W);
    }
  std::vector<uint32_t> size(HW, 0), line_max(HW, 0);
  for (uint32_t i = 0; i < HW; i++)
    if (cls[i] == kSegNode) {
      const uint32_t r = find_root(parent, i);
      size[r]++;
      if (i / W > line_max[r]) line_max[r] = i / W;
    }
  for (uint32_t i = 0; i < HW; i++) {
    labels[i] = kSegNoLabel, sizes[i] = 0, spans[i] = 0, classes[i] = cls[i];
    if (cls[i] != kSegNode) continue;
    const uint32_t r = find_root(parent, i);
    labels[i] = r, sizes[i] = size[r], spans[i] = line_max[r] - r / W + 1;
    classes[i] = seg_accepted(sizes[i], spans[i], P) ? kSegCluster : kSegOutlier;
  }
}

}  // extern "C"

#if defined(HOSTCHECK_SEGMENT_MAIN)
#include <math.h>
int main() {
  // generated scans at shapes around 1 and 2 lines / columns: walls at two ranges, holes, a floor, NaN and huge cells
  uint64_t s = 88172645463325252ull;
  auto rnd = [&]() {
    s ^= s << 13, s ^= s >> 7, s ^= s << 17;
    return (double)(s >> 11) / 9007199254740992.0;
  };
  const uint32_t shapes[][2] = {{1, 1}, {1, 2}, {2, 1}, {1, 16}, {5, 37}, {19, 300}, {32, 512}};
  unsigned long long total = 0;
  for (const auto& hw : shapes) {
    const uint32_t H = hw[0], W = hw[1], HW = H * W;
    std::vector<double> p(3 * (size_t)HW);
    for (uint32_t l = 0; l < H; l++)
      for (uint32_t c = 0; c < W; c++) {
        const double az = 2.0 * M_PI * c / W, el = (-20.0 + 2.0 * l) * M_PI / 180.0, u = rnd();
        double r = u < 0.4 ? 10.0 : u < 0.7 ? 20.0 : u < 0.8 ? 0.0 : u < 0.85 ? 1e30 : el < 0 ? 1.8 / -sin(el) : 50.0;
        double* q = &p[3 * (size_t)(l * W + c)];
        q[0] = r * cos(el) * cos(az), q[1] = r * cos(el) * sin(az), q[2] = r * sin(el);
        if (u > 0.99) q[1] = NAN;
      }
    std::vector<uint8_t> classes(HW);
    std::vector<uint32_t> labels(HW), sizes(HW), spans(HW);
    for (uint32_t g : {0u, 1u, 2u, H, H + 3})
      hostcheck_segment_scan(p.data(), H, W, g, 1.0, 120.0, 0.031, 0.25, 30, 5, 3, classes.data(), labels.data(), sizes.data(), spans.data());
    for (uint32_t i = 0; i < HW; i++) total += classes[i] + (labels[i] == kSegNoLabel ? 0u : labels[i]) + sizes[i] + spans[i];
    std::vector<uint8_t> out(HW);
    hostcheck_segment_valid(p.data(), HW, 1.0, 120.0, out.data());
    if (HW > 1) {
      hostcheck_segment_ground_pair(p.data(), p.data() + 3, HW - 1, 0.031, out.data());
      hostcheck_segment_connected(p.data(), p.data() + 3, HW - 1, 0.25, out.data());
    }
  }
  printf("hostcheck_segment ok %llu\n", total);
  return 0;
}
#endif
