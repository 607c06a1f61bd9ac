// crop_math.h — the rule of a map window (loamx.h, "map window"): the voxel bounds of a box around a centre, the decision to skip
// the crop, and whether a voxel key is kept. Host + device, like cloudmap_math.h, whose cell function the bounds repeat:
// tests/hostcheck_crop compiles this file with g++ and compares it with numpy. Every quotient and sum is rounded on its own
// (-ffp-contract=off).
#pragma once
#include "cloudmap_math.h"

namespace loamx {

// the bounds in voxel units, both inclusive; +-inf where a bound (or the sum with the centre) is infinite
struct CropBounds {
  double flo[3], fhi[3];
};

// a centre with a NaN or an infinite component skips the crop: the map keeps every byte
LOAMX_HD bool crop_skips(const double c[3]) { return !(cloud_finite(c[0]) && cloud_finite(c[1]) && cloud_finite(c[2])); }

// The cloud map's cell function (cloud_axis: floor(p / leaf) by an IEEE division) on the two corners of the box c + [lo, hi]. c is
// finite (crop_skips) and lo, hi are no NaN, so no bound is a NaN; a sum that overflows is +-inf and stays so.
LOAMX_HD CropBounds crop_bounds(const double c[3], const double lo[3], const double hi[3], double leaf) {
  CropBounds b;
  for (int a = 0; a < 3; a++) {
    b.flo[a] = floor((c[a] + lo[a]) / leaf);
    b.fhi[a] = floor((c[a] + hi[a]) / leaf);
  }
  return b;
}

// a voxel is kept iff its integer cell lies inside the bounds on all three axes: every point of the closed box lies in a kept cell
// (floor is monotonic), the box is widened to voxel boundaries and never narrowed
LOAMX_HD bool crop_keeps(uint64_t key, const CropBounds& b) {
  bool in = true;
  for (int a = 0; a < 3; a++) {
    const double v = (double)cloud_key_coord(key, a);
    in = in && v >= b.flo[a] && v <= b.fhi[a];
  }
  return in;
}

}  // namespace loamx
