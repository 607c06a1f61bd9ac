// distance_math.h — the rule of the occupancy distance field (loamx.h, "occupancy distance field"): which state is an obstacle,
// the pass along x on a row of mask words, the pass along y or z on a column of intermediates, in both early-exit forms, and the
// metres of a squared distance. Host + device: tests/hostcheck_distance compiles this file with g++ and compares it with numpy.
// Everything is integer but dist_metres, whose two operations are rounded each on its own (-ffp-contract=off); sqrt is the only
// libm call.
#pragma once
#include "occupancy_math.h"

namespace loamx {

constexpr uint32_t kDistFar = 0xFFFFu;      // LOAMX_DIST_FAR
constexpr uint32_t kDistMaxR = 255u;        // R^2 = 65025 < kDistFar
constexpr uint32_t kDistNone = 0xFFFFFFFFu;  // the cost of an intermediate that holds no obstacle
constexpr int32_t kDistNoDx = -32768;       // the x-pass found no obstacle within R
constexpr uint32_t kDistNoDxy = 0x80008000u;  // the y-pass found none (both halves kDistNoDx)

LOAMX_HD bool dist_obstacle(uint32_t state, bool unknown_is_obstacle) {
  return state == kOccOccupied || (unknown_is_obstacle && state == kOccUnknown);
}

// (dx, dy) of the y-pass in one dword: dx in the low half
LOAMX_HD uint32_t dist_pack(int32_t dx, int32_t dy) { return ((uint32_t)dx & 0xFFFFu) | ((uint32_t)dy << 16); }
LOAMX_HD int32_t dist_dx(uint32_t w) { return (int32_t)(int16_t)(uint16_t)(w & 0xFFFFu); }
LOAMX_HD int32_t dist_dy(uint32_t w) { return (int32_t)(int16_t)(uint16_t)(w >> 16); }
// what an intermediate costs before the pass adds its own k^2
LOAMX_HD uint32_t dist_cost_dx(int32_t dx) { return dx == kDistNoDx ? kDistNone : (uint32_t)(dx * dx); }
LOAMX_HD uint32_t dist_cost_dxy(uint32_t w) {
  const int32_t dx = dist_dx(w), dy = dist_dy(w);
  return dx == kDistNoDx ? kDistNone : (uint32_t)(dx * dx + dy * dy);
}

/* x-pass. `row`: the mask words of one row of the extended box, bit p of the row in word p >> 6 at bit p & 63; p: the voxel's
 * position in that row. The caller guarantees R <= p and p + R < 64 x (words of the row), which holds for every voxel of the box
 * (p = x + R, the row is dims[0] + 2R bits). Returns the signed offset to the nearest set bit within R, a tie to the left (the
 * lower x), kDistNoDx without one. At most R / 64 + 2 words each way. */
LOAMX_HD int32_t dist_x_pass(const unsigned long long* row, uint32_t p, uint32_t R) {
  uint32_t left = kDistNone, right = kDistNone;  // distances
  {  // the nearest set bit at a position <= p, down to p - R
    int32_t w = (int32_t)(p >> 6);
    const int32_t w_last = (int32_t)((p - R) >> 6);
    unsigned long long m = row[w] & (~0ull >> (63u - (p & 63u)));
    for (;;) {
      if (m) {
        left = p - ((uint32_t)w * 64u + 63u - (uint32_t)__builtin_clzll(m));
        break;
      }
      if (--w < w_last) break;
      m = row[w];
    }
    if (left > R) left = kDistNone;
  }
  if (left != 0u) {  // the nearest set bit at a position > p, up to p + R
    uint32_t w = (p + 1u) >> 6;
    const uint32_t w_last = (p + R) >> 6;
    unsigned long long m = row[w] & (~0ull << ((p + 1u) & 63u));
    for (;;) {
      if (m) {
        right = (uint32_t)w * 64u + (uint32_t)__builtin_ctzll(m) - p;
        break;
      }
      if (++w > w_last) break;
      m = row[w];
    }
    if (right > R) right = kDistNone;
  }
  if (left == kDistNone && right == kDistNone) return kDistNoDx;
  return left <= right ? -(int32_t)left : (int32_t)right;
}

/* y-pass and z-pass on one voxel. cost(k), k in -R .. R: what the intermediate k rows away from the voxel's own costs
 * (dist_cost_dx / dist_cost_dxy of it), kDistNone without an obstacle. The walk goes outwards k = 0, 1, 2, ..., the lower
 * coordinate first; the lower side is taken with <=, the higher with <: among equal costs the lowest coordinate wins. A cost
 * above R^2 is never taken. early: stop as soon as k^2 > best, which is exact, since a candidate at distance k costs at least
 * k^2; otherwise the whole window is walked. Returns the best cost (kDistNone: nothing within the cap) and its k. */
template <typename Cost>
LOAMX_HD uint32_t dist_column_pass(const Cost& cost, uint32_t R, bool early, int32_t& k_best) {
  const uint32_t cap = R * R;
  uint32_t best = cost(0);
  k_best = 0;
  if (best > cap) best = cap + 1u;  // "none": every real candidate beats it, and k^2 <= cap never stops the walk
  for (uint32_t k = 1; k <= R; k++) {
    const uint32_t kk = k * k;
    if (early && kk > best) break;
    const uint32_t lo = cost(-(int32_t)k), hi = cost((int32_t)k);
    if (lo != kDistNone && lo + kk <= cap && lo + kk <= best) best = lo + kk, k_best = -(int32_t)k;
    if (hi != kDistNone && hi + kk < best) best = hi + kk, k_best = (int32_t)k;
  }
  if (best > cap) {
    k_best = 0;
    return kDistNone;
  }
  return best;
}

// metres of a squared distance in voxels: +inf for kDistFar
LOAMX_HD float dist_metres(uint32_t d2, double leaf) {
  if (d2 == kDistFar) return (float)INFINITY;
  const double r = sqrt((double)d2);
  const double m = r * leaf;
  return (float)m;
}

}  // namespace loamx
