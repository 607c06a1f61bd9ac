// organize_math.h — where a point of an unordered cloud belongs in an organised scan (loamx.h: loamx_organize_clouds_dev): the
// validity test, the column against the table of column boundaries, the line against the table of boundary tangents or from a
// ring number. The rule itself is written out in loamx.h; tests/organize_common.py restates it in numpy with an n x W sign
// matrix and an n x (H + 1) comparison matrix, and the kernels must agree with that bit for bit. Hence every product and sum
// below is a statement of its own (the library and the hostcheck are compiled with -ffp-contract=off) and nothing here calls
// libm beyond sqrt, which is correctly rounded everywhere.
// Shared by host and device code like extract_math.h / reg_math.h / deskew_math.h.
#pragma once
#include <stdint.h>

#include "reg_math.h"

namespace loamx {

constexpr uint32_t kOrgCellInvalid = 0xFFFFFFFEu;  // no azimuth or not finite: dropped
constexpr uint32_t kOrgCellOutside = 0xFFFFFFFFu;  // outside the elevation fan, or a ring without a line: dropped
constexpr uint32_t kOrgNoRing = 0xFFFFFFFFu;       // `ring` of a call without ring numbers
constexpr double kOrgMinRho2 = 1e-100;

// the two tables of a scan layout and its shape
struct OrgTables {
  const double* col_dirs;    // [W][2]: u_k = (cos phi_k, sin phi_k), the direction of the boundary between columns k - 1 and k
  const double* line_tans;   // [H + 1]: tangent of the boundary below line l; ascending
  const uint16_t* ring_map;  // [n_ring_map] or nullptr
  uint32_t n_ring_map, H, W, clockwise;
};

// step 1 of the rule: rho2 and r2, and whether the point has a place at all
LOAMX_HD bool organize_valid(double x, double y, double z, double& rho2, double& r2) {
  const double xx = x * x, yy = y * y, zz = z * z;
  rho2 = xx + yy;
  r2 = rho2 + zz;
  const double big = 1.7976931348623157e308;
  const bool finite = fabs(x) <= big && fabs(y) <= big && fabs(z) <= big && fabs(r2) <= big;
  return finite && rho2 >= kOrgMinRho2;  // (a NaN fails both)
}

// s_k: the point lies within half a turn ahead of boundary k, in the sense the columns are counted
LOAMX_HD bool organize_side(const OrgTables& t, uint32_t k, double x, double y) {
  const double a = t.col_dirs[2 * k] * y, b = t.col_dirs[2 * k + 1] * x;
  const double c = a - b;
  return (t.clockwise ? -c : c) >= 0.0;
}

// Step 2: the column c with s_c true and s_(c + 1) mod W false. Seen along k the signs are one run of about W / 2 trues and one
// of falses, cyclically. With m = W / 2, boundaries 0 .. m lie within half a turn ahead of boundary 0 and m .. W - 1 within half
// a turn behind it, so s_0 and s_m say in which of the two ranges the run of trues ends, and inside that range the signs are
// T .. T F .. F: a bisection between an index that WAS true and one that WAS false. The two cases in which s_0 and s_m do not
// bracket the end (a point within rounding of the direction opposite boundary 0, or W <= 2) walk from m until they stand on
// it. Whatever comes back has s_c true and s_(c + 1) false as computed — wherever the rule's c is unique, this is it — unless
// all W signs agree, which takes a W <= 2; then the walk ends where it started and the column is m.
LOAMX_HD uint32_t organize_column(const OrgTables& t, double x, double y) {
  const uint32_t W = t.W;
  if (W == 1) return 0;
  const uint32_t m = W / 2;
  const bool s0 = organize_side(t, 0, x, y), sm = organize_side(t, m, x, y);
  if (s0 != sm) {
    uint32_t lo = s0 ? 0u : m, hi = s0 ? m : W;  // s_lo true, s_hi false (s_W is s_0)
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (organize_side(t, mid, x, y)) lo = mid;
      else hi = mid;
    }
    return lo;
  }
  uint32_t c = m;
  if (s0) {  // both true: forward to the last true
    for (uint32_t i = 0; i < W; i++) {
      const uint32_t n = c + 1 == W ? 0u : c + 1;
      if (!organize_side(t, n, x, y)) break;
      c = n;
    }
  } else {  // both false: back to the first true
    for (uint32_t i = 0; i < W; i++) {
      c = c == 0 ? W - 1 : c - 1;
      if (organize_side(t, c, x, y)) break;
    }
  }
  return c;
}

// Step 3 without rings: cnt = the number of l in 0 .. H with z >= t_l rho, found as the first l for which that fails (the
// tangents ascend and rho > 0, so the answers are T .. T F .. F); H + 1 if none fails
LOAMX_HD uint32_t organize_line_count(const OrgTables& t, double rho2, double z) {
  const double rho = sqrt(rho2);
  uint32_t lo = 0, hi = t.H + 1;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    const double lim = t.line_tans[mid] * rho;
    if (z >= lim) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the whole rule for one point: its cell line * W + column, or kOrgCellInvalid / kOrgCellOutside; r2 for KEEP_NEAREST
LOAMX_HD uint32_t organize_cell(const OrgTables& t, double x, double y, double z, uint32_t ring, double& r2) {
  double rho2;
  if (!organize_valid(x, y, z, rho2, r2)) return kOrgCellInvalid;
  const uint32_t col = organize_column(t, x, y);
  uint32_t line;
  if (ring == kOrgNoRing) {
    const uint32_t cnt = organize_line_count(t, rho2, z);
    if (cnt == 0 || cnt == t.H + 1) return kOrgCellOutside;
    line = cnt - 1;
  } else {
    line = ring;
    if (t.ring_map) {
      if (ring >= t.n_ring_map) return kOrgCellOutside;
      line = t.ring_map[ring];
      if (line == 0xFFFFu) return kOrgCellOutside;
    }
    if (line >= t.H) return kOrgCellOutside;
  }
  return line * t.W + col;
}

// ---- the two tables, made once per scan layout: HOST functions (FP64, libm) ------------------------------------------------------
// u_k = (cos phi_k, sin phi_k), phi_k = azimuth_zero + sgn 2 pi (k - 1/2) / W; col_dirs: [W][2]
inline void organize_column_dirs(double azimuth_zero, bool clockwise, uint32_t W, double* col_dirs) {
  const double sgn = clockwise ? -1.0 : 1.0, two_pi = 6.283185307179586476925286766559;
  for (uint32_t k = 0; k < W; k++) {
    const double phi = azimuth_zero + sgn * (two_pi * ((double)k - 0.5) / (double)W);
    col_dirs[2 * k] = cos(phi), col_dirs[2 * k + 1] = sin(phi);
  }
}
// the beam elevations of a layout without an explicit list: linear from fov_bottom (line 0) to fov_top (line H - 1); H >= 2
inline double organize_linear_elevation(double fov_bottom, double fov_top, uint32_t H, uint32_t line) {
  return fov_bottom + (fov_top - fov_bottom) * (double)line / (double)(H - 1);
}
// line_tans[H + 1] from the H beam elevations (radians, line 0 the lowest): the tangents of the elevations half way between
// neighbouring beams, the two outer ones half the adjacent spacing beyond the outer beams; H == 1: {-inf, +inf}. Returns
// nullptr, or why the elevations are refused.
inline const char* organize_line_tans(const double* elevations, uint32_t H, double* line_tans) {
  const double big = 1.7976931348623157e308, half_pi = 1.5707963267948966192313216916398;
  for (uint32_t i = 0; i < H; i++) {
    if (!(fabs(elevations[i]) <= big)) return "an elevation is not finite";
    if (i > 0 && !(elevations[i] > elevations[i - 1])) return "the elevations must ascend strictly";
  }
  if (H == 1) {
    line_tans[0] = -INFINITY, line_tans[1] = INFINITY;
    return nullptr;
  }
  for (uint32_t i = 0; i <= H; i++) {
    double b;
    if (i == 0) b = elevations[0] - (elevations[1] - elevations[0]) / 2.0;
    else if (i == H) b = elevations[H - 1] + (elevations[H - 1] - elevations[H - 2]) / 2.0;
    else b = (elevations[i - 1] + elevations[i]) / 2.0;
    if (!(b > -half_pi && b < half_pi)) return "a boundary elevation lies outside (-pi/2, pi/2)";
    line_tans[i] = tan(b);
  }
  return nullptr;
}

}  // namespace loamx
