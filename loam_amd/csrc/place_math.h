// place_math.h — the arithmetic of place recognition (loamx.h, "place recognition"): where a point falls in the polar grid of a
// scan descriptor and with which height code, the quantised cosine of two descriptor columns from their integer sums, the
// distance of a shift from its integer score. The rule itself is written out in loamx.h; tests/place_common.py restates it in
// numpy and the kernels must agree with that byte for byte. Hence every product and sum below is a statement of its own (the
// library and the hostcheck are compiled with -ffp-contract=off), every accumulation is an integer one, and nothing here calls
// libm beyond sqrt and floor, which are exact everywhere.
// Shared by host and device code like organize_math.h, whose validity test and column search it uses as they stand.
#pragma once
#include <stdint.h>

#include "organize_math.h"

namespace loamx {

constexpr uint32_t kPlaceNoCell = 0xFFFFFFFFu;       // the point is dropped: invalid, or at / beyond max_range
constexpr uint32_t kPlaceMaxRings = 64, kPlaceMinSectors = 3, kPlaceMaxSectors = 360;
constexpr uint32_t kPlaceMaxCandidates = 64;
constexpr uint32_t kPlaceMaxHeight = 65534;          // largest h; codes are h + 1 = 1 .. 65535, 0 is "no point"
constexpr uint64_t kPlaceCosOne = 1ull << 30;        // the quantised cosine 1.0
constexpr uint32_t kPlaceNoId = 0xFFFFFFFFu;         // id of a record without an entry
constexpr uint64_t kPlaceNoKeyDist = ~0ull;          // its key distance (a real one is < 2^63)
constexpr uint32_t kPlaceMaxEntries = 1u << 24;

// the shape of a descriptor and the three scalars of the per-point rule
struct PlaceShape {
  uint32_t R, S;
  double ring_scale;  // R / max_range, formed once on the host
  double z_offset, z_scale;
};

// step 4 of the rule: h = floor((z + z_offset) z_scale) clamped to [0, 65534], code = h + 1
LOAMX_HD uint32_t place_code(const PlaceShape& p, double z) {
  const double a = z + p.z_offset;
  const double b = a * p.z_scale;
  const double h = floor(b);
  if (!(h >= 0.0)) return 1u;  // (z_offset finite, z_scale finite and positive, z finite: b is never a NaN)
  if (h >= (double)kPlaceMaxHeight) return kPlaceMaxHeight + 1u;
  return (uint32_t)h + 1u;
}

// steps 1 - 4 for one point: its cell ring * S + sector with its code, or kPlaceNoCell. dirs: the S sector boundaries [S][2]
LOAMX_HD uint32_t place_cell(const PlaceShape& p, const double* dirs, double x, double y, double z, uint32_t& code) {
  double rho2, r2;
  if (!organize_valid(x, y, z, rho2, r2)) return kPlaceNoCell;
  const double rho = sqrt(rho2);
  const double f = rho * p.ring_scale;
  if (!(f < (double)p.R)) return kPlaceNoCell;
  const uint32_t ring = (uint32_t)floor(f);
  const OrgTables t{dirs, nullptr, nullptr, 0u, 0u, p.S, 0u};
  const uint32_t sector = organize_column(t, x, y);
  code = place_code(p, z);
  return ring * p.S + sector;
}

// k_j: the cosine of two columns with the exact dot product `dot` and the non-zero squared norms nq, ne, in units of 2^-30.
// The norms are multiplied before the root is taken: sqrt(fl(n n)) is n for every integer n < 2^53, so a column against itself
// has the cosine 1.0 exactly, which sqrt(n) sqrt(n) misses for most n (n = 2: 2 / 2.0000000000000004).
LOAMX_HD uint64_t place_cos_q(uint64_t dot, uint64_t nq, uint64_t ne) {
  const double prod = (double)nq * (double)ne;
  const double den = sqrt(prod);
  const double c = (double)dot / den;
  const double t = c * (double)kPlaceCosOne;
  if (!(t < (double)kPlaceCosOne)) return kPlaceCosOne;  // (the minimum is taken before the cast: no double out of uint64's range is converted)
  return (uint64_t)floor(t);
}

// dist(s) from the integer score of a shift and the number m of columns that counted
LOAMX_HD double place_shift_distance(uint64_t score, uint32_t m) {
  if (m == 0) return 1.0;
  const double den = (double)m * (double)kPlaceCosOne;
  const double q = (double)score / den;
  return 1.0 - q;
}

}  // namespace loamx
