// map_math.h — per-point arithmetic of the map upkeep (loamx.h, "map upkeep"): the voxel of a point, its 63-bit key, the
// slot the key hashes to and the box test of the crop. Host + device, like reg_math.h: tests/hostcheck_map compiles this
// file with g++ and compares it with numpy.
#pragma once
#include "reg_math.h"

namespace loamx {

constexpr double kVoxelRange = 1048576.0;      // |floor(p / leaf)| must stay below 2^20 on every axis
constexpr uint64_t kVoxelEmpty = ~(uint64_t)0;  // no key looks like this: a key has 63 bits

// One axis: v = floor(p / leaf) by an IEEE division (NOT p * (1 / leaf): a point on a voxel face must land where
// numpy.floor(p / leaf) puts it), biased by 2^20 into 21 bits. false: NaN, infinite or out of range.
LOAMX_HD bool voxel_coord(double p, double leaf, uint64_t& biased) {
  const double v = floor(p / leaf);
  if (!(fabs(v) < kVoxelRange)) return false;
  biased = (uint64_t)((int64_t)v + 1048576);
  return true;
}
LOAMX_HD uint64_t voxel_pack(uint64_t bx, uint64_t by, uint64_t bz) { return bx << 42 | by << 21 | bz; }
LOAMX_HD bool voxel_key(Vec3 p, double leaf, uint64_t& key) {
  uint64_t bx = 0, by = 0, bz = 0;
  const bool ok = voxel_coord(p.x, leaf, bx) & voxel_coord(p.y, leaf, by) & voxel_coord(p.z, leaf, bz);
  key = voxel_pack(bx, by, bz);
  return ok;
}
// multiplicative (Fibonacci) hash to log2_cap bits, 4 <= log2_cap <= 32: the first slot of the key's probe sequence
LOAMX_HD uint32_t voxel_hash(uint64_t key, uint32_t log2_cap) { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64u - log2_cap)); }

// exactly {0, 0, 0, 1, 0, 0, 0}: the transform is skipped, so that the points come back bit for bit (quat_rotate would turn
// a -0.0 coordinate into +0.0)
LOAMX_HD bool pose_is_identity(const double P[7]) {
  return P[0] == 0.0 && P[1] == 0.0 && P[2] == 0.0 && P[3] == 1.0 && P[4] == 0.0 && P[5] == 0.0 && P[6] == 0.0;
}

// lo[c] <= p[c] <= hi[c] on every axis (a NaN coordinate is outside)
LOAMX_HD bool box_holds(Vec3 p, const double lo[3], const double hi[3]) {
  return p.x >= lo[0] && p.x <= hi[0] && p.y >= lo[1] && p.y <= hi[1] && p.z >= lo[2] && p.z <= hi[2];
}

}  // namespace loamx
