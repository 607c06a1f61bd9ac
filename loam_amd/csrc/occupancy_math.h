// occupancy_math.h — per-ray arithmetic of the occupancy map (loamx.h, "occupancy map"): which rays count, their end points, the
// hit voxel, the set-up and the step of the voxel walk, and the state of a voxel's two counts. Host + device, like
// cloudmap_math.h, whose validity tests, voxel rule and key packing it reuses: tests/hostcheck_occupancy compiles this file with
// g++ and compares it with numpy. FP64 throughout; every product, quotient, sum and difference is rounded on its own
// (-ffp-contract=off); the only libm call is sqrt.
#pragma once
#include "cloudmap_math.h"

namespace loamx {

enum { kOccUnknown = 0, kOccFree = 1, kOccOccupied = 2 };  // LOAMX_OCC_*
// what becomes of a ray at step 1
enum { kOccRayNormal = 0, kOccRayInvalid = 1, kOccRayShort = 2, kOccRayLong = 3 };

constexpr uint64_t kOccMaxOffered = 0xFFFFFFFEull;  // rays offered between two clears: neither half of a count word can wrap
constexpr uint64_t kOccHitUnit = 1ull << 32;        // a count word is hits << 32 | passes

struct OccRule {
  double leaf, min_r2, max_r2;  // the squares are formed once by the host
  double max_range, end_margin;
  uint32_t clip_long;
};
struct OccStateRule {
  uint32_t min_hits, min_passes;
  double occ_ratio;
};

// step 5
LOAMX_HD uint32_t occ_state(uint32_t hits, uint32_t passes, const OccStateRule& s) {
  if (hits >= s.min_hits && (double)hits >= s.occ_ratio * (double)passes) return kOccOccupied;
  return passes >= s.min_passes ? kOccFree : kOccUnknown;
}

// step 1: cloud_validity's tests, with the two range failures told apart
LOAMX_HD int occ_classify(Vec3 p, double min_r2, double max_r2, double& r2) {
  r2 = p.x * p.x + p.y * p.y + p.z * p.z;
  if (!(cloud_finite(p.x) && cloud_finite(p.y) && cloud_finite(p.z) && cloud_finite(r2))) return kOccRayInvalid;
  if (!(r2 >= min_r2)) return kOccRayShort;
  if (!(r2 <= max_r2)) return kOccRayLong;
  return kOccRayNormal;
}

// the voxel walk of one ray: the voxel it stands in (biased into 21 bits per axis, as the key packs them), the steps left per
// axis, and the two parameters per axis of step 4. Indexed by constants only (the loops below unroll), so it lives in registers.
struct OccWalk {
  uint32_t b[3];    // v + 2^20
  uint32_t rem[3];  // |ve - v|
  int32_t dir[3];
  double t_max[3], t_delta[3];
};
LOAMX_HD uint64_t occ_walk_key(const OccWalk& w) { return voxel_pack(w.b[0], w.b[1], w.b[2]); }
LOAMX_HD uint32_t occ_walk_steps(const OccWalk& w) { return w.rem[0] + w.rem[1] + w.rem[2]; }

// step 4 on one axis, from the walk's two end points; false: a voxel coordinate outside |v| < 2^20 (or not a number)
LOAMX_HD bool occ_walk_axis(double o, double e, double leaf, uint32_t& b, uint32_t& rem, int32_t& dir, double& t_max, double& t_delta) {
  const double to = o / leaf, te = e / leaf;
  const double v = floor(to), ve = floor(te);
  b = 0, rem = 0, dir = 1, t_max = 0.0, t_delta = 0.0;
  if (!(fabs(v) < kVoxelRange) || !(fabs(ve) < kVoxelRange)) return false;
  const int32_t iv = (int32_t)v, ive = (int32_t)ve;
  b = (uint32_t)(iv + 1048576);
  dir = ive >= iv ? 1 : -1;
  rem = (uint32_t)(ive >= iv ? ive - iv : iv - ive);
  if (rem > 0) {
    const double ad = fabs(te - to);
    t_delta = 1.0 / ad;
    t_max = (dir > 0 ? (v + 1.0) - to : to - v) / ad;
  }
  return true;
}
LOAMX_HD bool occ_walk_begin(Vec3 o, Vec3 e, double leaf, OccWalk& w) {
  const bool okx = occ_walk_axis(o.x, e.x, leaf, w.b[0], w.rem[0], w.dir[0], w.t_max[0], w.t_delta[0]);
  const bool oky = occ_walk_axis(o.y, e.y, leaf, w.b[1], w.rem[1], w.dir[1], w.t_max[1], w.t_delta[1]);
  const bool okz = occ_walk_axis(o.z, e.z, leaf, w.b[2], w.rem[2], w.dir[2], w.t_max[2], w.t_delta[2]);
  return okx & oky & okz;
}
// one step (the caller counts them: occ_walk_steps before the first): among the axes with steps left the one with the smallest
// t_max, ties to the lowest axis
LOAMX_HD void occ_walk_step(OccWalk& w) {
  int pick = -1;
  double best = 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int a = 0; a < 3; a++)
    if (w.rem[a] > 0 && (pick < 0 || w.t_max[a] < best)) pick = a, best = w.t_max[a];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int a = 0; a < 3; a++)
    if (pick == a) {
      w.b[a] = (uint32_t)((int32_t)w.b[a] + w.dir[a]);
      w.t_max[a] = w.t_max[a] + w.t_delta[a];
      w.rem[a] -= 1u;
    }
}

// steps 1 to 4 up to the walk's first voxel
struct OccRay {
  int kind;          // kOccRay*
  bool has_hit;      // hits[hit_key] += 1
  bool outside;      // counted `outside` (a ray dropped whole, or a walk that is not taken)
  bool walks;        // w is set up: visit occ_walk_key, then occ_walk_steps steps
  uint64_t hit_key;  // valid while has_hit
  OccWalk w;
};
// pose: 7 doubles (qx qy qz qw tx ty tz), read only when `posed`; otherwise no transform, origin 0
LOAMX_HD void occ_ray(Vec3 p, bool posed, const double pose[7], const OccRule& R, OccRay& r) {
  double r2;
  r.kind = occ_classify(p, R.min_r2, R.max_r2, r2);
  r.has_hit = r.outside = r.walks = false;
  r.hit_key = 0;
  if (r.kind == kOccRayInvalid || r.kind == kOccRayShort) return;
  const bool is_long = r.kind == kOccRayLong;
  if (is_long && !R.clip_long) return;
  Vec3 q = p, o = v3(0.0, 0.0, 0.0);
  if (posed) q = pose_act(pose, p), o = v3(pose[4], pose[5], pose[6]);
  const Vec3 d = vsub(q, o);
  const double dist = sqrt(r2);
  const double s = is_long ? R.max_range / dist : (dist - R.end_margin) / dist;
  if (!is_long) {
    uint32_t u[3];
    if (!cloud_cell(q, R.leaf, r.hit_key, u)) {
      r.outside = true;
      return;
    }
    r.has_hit = true;
  }
  if (!(s > 0.0)) return;
  const Vec3 e = v3(o.x + s * d.x, o.y + s * d.y, o.z + s * d.z);
  if (occ_walk_begin(o, e, R.leaf, r.w)) r.walks = true;
  else r.outside = true;
}

}  // namespace loamx
