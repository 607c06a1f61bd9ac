// visibility_math.h — the visibility vote of a map point in a scan (loamx.h, "map cleaning"): the point into the sensor frame,
// its cell by the organiser's rule, the range band around it, the verdict over the window of cells, and the decision over a
// point's votes. The rule itself is written out in loamx.h; tests/visibility_common.py restates it in numpy and the kernels
// (visibility_kernels.hip) must agree with that bit for bit. Hence every product, sum and difference below is a statement
// of its own (the library and the hostcheck are compiled with -ffp-contract=off) and nothing here calls libm beyond sqrt.
// Shared by host and device code like organize_math.h / cloudmap_math.h.
#pragma once
#include <stdint.h>

#include "organize_math.h"

namespace loamx {

// verdicts in the order of the fields of loamx_visibility_tally; kVisNone counts nowhere
enum { kVisThrough = 0, kVisAgree = 1, kVisOccluded = 2, kVisEmpty = 3, kVisNone = 4 };
// how far a (point, scan) pair came: kVisPlaceNone failed step 2, kVisPlaceInRange passed it, kVisPlaceProjected has a cell
enum { kVisPlaceNone = 0, kVisPlaceInRange = 1, kVisPlaceProjected = 2 };

// loamx_visibility_params as the kernels take it: the squares formed once per call on the host
struct VisRule {
  double min2, max2, margin, margin_rel;
  uint32_t window_lines, window_cols;
};

// step 1: p = conj(q) (m - t), the quaternion of world_T_s used as given
LOAMX_HD Vec3 vis_to_sensor(const double P[7], Vec3 m) {
  const Vec3 d = vsub(m, v3(P[4], P[5], P[6]));
  const double qc[4] = {-P[0], -P[1], -P[2], P[3]};
  return quat_rotate(qc, d);
}

// steps 2 and 3: whether the point has a place in the scan, and its cell
LOAMX_HD int vis_place(const OrgTables& t, Vec3 p, const VisRule& rule, uint32_t& cell, double& r2) {
  double rho2;
  cell = kOrgCellOutside;
  if (!organize_valid(p.x, p.y, p.z, rho2, r2)) return kVisPlaceNone;
  if (!(r2 >= rule.min2) || !(r2 <= rule.max2)) return kVisPlaceNone;
  cell = organize_cell(t, p.x, p.y, p.z, kOrgNoRing, r2);
  return cell == kOrgCellOutside || cell == kOrgCellInvalid ? kVisPlaceInRange : kVisPlaceProjected;
}

// step 4: the squared range band [lo2, hi2] around a point at squared range r2
LOAMX_HD void vis_bounds(double r2, const VisRule& rule, double& lo2, double& hi2) {
  const double dist = sqrt(r2);
  const double rel = rule.margin_rel * dist;
  const double tol = rule.margin + rel;
  double lo = dist - tol;
  if (lo < 0.0) lo = 0.0;
  const double hi = dist + tol;
  lo2 = lo * lo, hi2 = hi * hi;
}

// a scan cell's squared range, or -1 for a cell that is not usable (a coordinate not finite, or nearer than min_range)
LOAMX_HD double vis_cell_r2(double x, double y, double z, double min2) {
  const double xx = x * x, yy = y * y, zz = z * z;
  const double rho2 = xx + yy;
  const double r2c = rho2 + zz;
  const bool finite = fabs(x) <= kDblMax && fabs(y) <= kDblMax && fabs(z) <= kDblMax;
  return finite && r2c >= min2 ? r2c : -1.0;
}

// steps 5 and 6: the verdict over the window around cell (l, c); r2_of(i) is vis_cell_r2 of cell i of the scan. Lines are
// clipped, columns wrap; a cell met twice changes nothing (the reductions are `any` and `all`).
template <typename F>
LOAMX_HD int vis_window(uint32_t l, uint32_t c, uint32_t H, uint32_t W, const VisRule& rule, double lo2, double hi2, F r2_of) {
  bool usable = false, agree = false, all_beyond = true;
  const int wl = (int)rule.window_lines, wc = (int)rule.window_cols;
  for (int dl = -wl; dl <= wl; dl++) {
    const long long ll = (long long)l + dl;
    if (ll < 0 || ll >= (long long)H) continue;
    for (int dc = -wc; dc <= wc; dc++) {
      long long cc = ((long long)c + dc) % (long long)W;  // (|dc| <= 3, W >= 1)
      if (cc < 0) cc += W;
      const double r2c = r2_of((uint32_t)ll * W + (uint32_t)cc);
      if (!(r2c >= 0.0)) continue;
      usable = true;
      if (r2c >= lo2 && r2c <= hi2) agree = true;
      if (!(r2c > hi2)) all_beyond = false;
    }
  }
  if (!usable) return kVisEmpty;
  if (agree) return kVisAgree;
  return all_beyond ? kVisThrough : kVisOccluded;
}

// the whole rule for one map point and one scan of scalar type T (H W x 3), at pose P = world_T_s; *place: kVisPlace*
template <typename T>
LOAMX_HD int vis_verdict(const OrgTables& t, const VisRule& rule, const double P[7], Vec3 m, const T* scan, int* place) {
  const Vec3 p = vis_to_sensor(P, m);
  uint32_t cell;
  double r2;
  *place = vis_place(t, p, rule, cell, r2);
  if (*place != kVisPlaceProjected) return kVisNone;
  double lo2, hi2;
  vis_bounds(r2, rule, lo2, hi2);
  const double min2 = rule.min2;
  return vis_window(cell / t.W, cell % t.W, t.H, t.W, rule, lo2, hi2, [scan, min2](uint32_t i) {
    const T* q = scan + (size_t)i * 3;
    return vis_cell_r2((double)q[0], (double)q[1], (double)q[2], min2);
  });
}

// the decision over a point's votes: one rounded product
LOAMX_HD bool vis_dynamic(uint32_t through, uint32_t agree, uint32_t min_through, double through_ratio) {
  const double need = through_ratio * (double)agree;
  return through >= min_through && (double)through >= need;
}

}  // namespace loamx
