// TEST-ONLY: visibility_math.h (the per-pair arithmetic of the map cleaning kernels) compiled for the host behind extern "C"
// wrappers, for tests/test_visibility_hostcheck.py. With -DHOSTCHECK_VISIBILITY_MAIN the file is a stand-alone program that votes
// generated points over generated scans with the same functions (the `san` target builds it with -fsanitize=address,undefined).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../loam_amd/csrc/visibility_math.h"

using namespace loamx;

struct Tally {
  uint32_t through, agree, occluded, empty;
};

extern "C" {

// verdict[i] (kVis*) and place[i] (kVisPlace*) of pts[i] (n x 3, world) in one scan (H W x 3, float when f32) at `pose`;
// rule = {min2, max2, margin, margin_rel}
void hostcheck_visibility_verdicts(const double* pts, uint64_t n, const void* scan, int f32, const double* pose, uint32_t H, uint32_t W,
                                   const double* col_dirs, const double* line_tans, uint32_t clockwise, const double* rule, uint32_t window_lines,
                                   uint32_t window_cols, int32_t* verdict, int32_t* place) {
  const OrgTables t{col_dirs, line_tans, nullptr, 0u, H, W, clockwise};
  const VisRule r{rule[0], rule[1], rule[2], rule[3], window_lines, window_cols};
  for (uint64_t i = 0; i < n; i++) {
    const Vec3 m = v3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
    int pl = 0;
    verdict[i] = f32 ? vis_verdict(t, r, pose, m, static_cast<const float*>(scan), &pl) : vis_verdict(t, r, pose, m, static_cast<const double*>(scan), &pl);
    place[i] = pl;
  }
}

void hostcheck_visibility_dynamic(const Tally* votes, uint64_t n, uint32_t min_through, double through_ratio, uint8_t* out) {
  for (uint64_t i = 0; i < n; i++) out[i] = vis_dynamic(votes[i].through, votes[i].agree, min_through, through_ratio) ? 1 : 0;
}

}  // extern "C"

#ifdef HOSTCHECK_VISIBILITY_MAIN
#include <math.h>
int main() {
  // a sensor inside a sphere of radius 20 with holes (zero and NaN cells), map points on, inside and outside the sphere and
  // outside the fan, a handful of poses, every window up to 3 x 3 cells each way, at widths that make the window lap itself
  uint64_t state = 88172645463325252ull;
  auto rnd = [&]() {
    state ^= state << 13, state ^= state >> 7, state ^= state << 17;
    return (double)(state >> 11) / 9007199254740992.0;
  };
  unsigned long long seen[5] = {0, 0, 0, 0, 0};
  const uint32_t shapes[][2] = {{16, 256}, {5, 37}, {2, 4}, {3, 1}, {4, 2}};
  for (const auto& shape : shapes) {
    const uint32_t H = shape[0], W = shape[1];
    std::vector<double> col(2 * (size_t)W), tans((size_t)H + 1), el(H);
    organize_column_dirs(0.1, false, W, col.data());
    for (uint32_t l = 0; l < H; l++) el[l] = organize_linear_elevation(-0.4, 0.3, H, l);
    if (organize_line_tans(el.data(), H, tans.data())) return 2;
    std::vector<float> scan(3 * (size_t)H * W);
    for (uint32_t l = 0; l < H; l++)
      for (uint32_t c = 0; c < W; c++) {
        const double az = 0.1 + 6.283185307179586 * c / W, e = el[l], r = 20.0 + 0.01 * rnd();
        float* q = &scan[3 * ((size_t)l * W + c)];
        q[0] = (float)(r * cos(e) * cos(az)), q[1] = (float)(r * cos(e) * sin(az)), q[2] = (float)(r * sin(e));
        const double hole = rnd();
        if (hole < 0.05) q[0] = q[1] = q[2] = 0.0f;
        else if (hole < 0.08) q[1] = NAN;
      }
    std::vector<double> pts;
    for (int i = 0; i < 4000; i++) {
      const double az = 6.283185307179586 * rnd(), e = -0.6 + 1.1 * rnd(), r = 0.2 + 30.0 * rnd();
      pts.insert(pts.end(), {r * cos(e) * cos(az), r * cos(e) * sin(az), r * sin(e)});
    }
    pts.insert(pts.end(), {0.0, 0.0, 0.0, 0.0, 0.0, 5.0, NAN, 1.0, 1.0, INFINITY, 0.0, 0.0, 1e200, 1e200, 0.0, 20.0, 0.0, 0.0});
    const uint64_t n = pts.size() / 3;
    const double poses[][7] = {{0, 0, 0, 1, 0, 0, 0}, {0, 0, 0.1, 0.99, 0.5, -0.25, 0.1}, {0.2, -0.1, 0.3, 1.7, 1.0, 2.0, -0.5}};
    std::vector<int32_t> verdict(n), place(n);
    for (const auto& pose : poses)
      for (uint32_t wl = 0; wl <= 3; wl++)
        for (uint32_t wc = 0; wc <= 3; wc++) {
          const double rule[4] = {1.0, 6400.0, 0.3, 0.01};
          hostcheck_visibility_verdicts(pts.data(), n, scan.data(), 1, pose, H, W, col.data(), tans.data(), 0, rule, wl, wc, verdict.data(), place.data());
          for (uint64_t i = 0; i < n; i++) {
            if (verdict[i] < 0 || verdict[i] > kVisNone || (verdict[i] != kVisNone) != (place[i] == kVisPlaceProjected)) {
              printf("point %llu: verdict %d with place %d\n", (unsigned long long)i, verdict[i], place[i]);
              return 1;
            }
            seen[verdict[i]]++;
          }
        }
  }
  for (int k = 0; k < 5; k++)
    if (!seen[k]) {
      printf("the inputs no longer reach verdict %d\n", k);
      return 1;
    }
  const Tally votes[] = {{2, 2, 0, 0}, {1, 0, 0, 0}, {3, 4, 0, 0}, {0, 0, 0, 0}, {0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0}};
  uint8_t dyn[5];
  hostcheck_visibility_dynamic(votes, 5, 2, 1.0, dyn);
  if (!(dyn[0] == 1 && dyn[1] == 0 && dyn[2] == 0 && dyn[3] == 0 && dyn[4] == 1)) {
    printf("the decision rule\n");
    return 1;
  }
  printf("hostcheck_visibility ok: through %llu agree %llu occluded %llu empty %llu none %llu\n", seen[0], seen[1], seen[2], seen[3], seen[4]);
  return 0;
}
#endif
