// cloudmap_math.h — per-point arithmetic of the cloud map (loamx.h, "cloud map"): which points count, the voxel of a point with
// the 32-bit fixed-point offset inside it, and the centroid of a voxel's integer sums. Host + device, like map_math.h, whose
// voxel key it reuses: tests/hostcheck_cloudmap compiles this file with g++ and compares it with numpy. Every product,
// quotient, sum and difference is rounded on its own (-ffp-contract=off).
#pragma once
#include "map_math.h"

namespace loamx {

// what becomes of a point (the words of the map's counters follow the same order)
enum { kCloudUsed = 0, kCloudInvalid = 1, kCloudRange = 2, kCloudOutside = 3 };

constexpr double kCloudUnit = 4294967296.0;    // offsets inside a voxel count in steps of leaf / 2^32
constexpr uint64_t kCloudMaxOffered = 0xFFFFFFFEull;  // points offered between two clears: no count and no sum can wrap

// finite (NaN and both infinities fail the subtraction test)
LOAMX_HD bool cloud_finite(double v) { return v - v == 0.0; }

// step 1 of the rule: kCloudInvalid for a non-finite coordinate or squared range, kCloudRange outside [min_r2, max_r2] (the two
// squares are formed once by the host), kCloudUsed otherwise
LOAMX_HD int cloud_validity(Vec3 p, double min_r2, double max_r2) {
  const double r2 = p.x * p.x + p.y * p.y + p.z * p.z;
  if (!(cloud_finite(p.x) && cloud_finite(p.y) && cloud_finite(p.z) && cloud_finite(r2))) return kCloudInvalid;
  if (!(r2 >= min_r2) || !(r2 <= max_r2)) return kCloudRange;
  return kCloudUsed;
}

// steps 3 and 4 on one axis: t = p / leaf, v = floor(t) biased as voxel_coord does, u = floor((t - v) 2^32) clamped to
// 2^32 - 1 (t = -1e-20 has v = -1 and t - v == 1.0 exactly). false: NaN, infinite or |v| >= 2^20.
LOAMX_HD bool cloud_axis(double p, double leaf, uint64_t& biased, uint32_t& u) {
  const double t = p / leaf;
  const double v = floor(t);
  if (!(fabs(v) < kVoxelRange)) return false;
  biased = (uint64_t)((int64_t)v + 1048576);
  const double frac = t - v;
  const uint64_t w = (uint64_t)floor(frac * kCloudUnit);
  u = w > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)w;
  return true;
}
LOAMX_HD bool cloud_cell(Vec3 p, double leaf, uint64_t& key, uint32_t u[3]) {
  uint64_t bx = 0, by = 0, bz = 0;
  u[0] = u[1] = u[2] = 0;
  const bool ok = cloud_axis(p.x, leaf, bx, u[0]) & cloud_axis(p.y, leaf, by, u[1]) & cloud_axis(p.z, leaf, bz, u[2]);
  key = voxel_pack(bx, by, bz);
  if (!ok) u[0] = u[1] = u[2] = 0;  // (the axes that had a voxel left their offsets: a point without a voxel carries none)
  return ok;
}

// voxel coordinate of axis a (0 x, 1 y, 2 z) of a key
LOAMX_HD int64_t cloud_key_coord(uint64_t key, int a) { return (int64_t)((key >> (42 - 21 * a)) & 0x1FFFFFull) - 1048576; }

// step 6 on one axis
LOAMX_HD double cloud_centroid(int64_t v, uint64_t sum, uint32_t count, double leaf) {
  return ((double)v + ((double)sum / (double)count) / kCloudUnit) * leaf;
}

}  // namespace loamx
