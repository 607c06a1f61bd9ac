// raycast_math.h — per-ray arithmetic of the occupancy ray cast (loamx.h, "occupancy ray casting"): the validity of a segment, the
// walk of occupancy_math.h with the parameter at which every voxel is entered and left, the test of a visited voxel, the step cap,
// the 40-byte record, and the beam and the return of a rendered scan. Host + device, like occupancy_math.h, whose walk it takes
// unchanged: tests/hostcheck_raycast compiles this file with g++ and compares it with a Python model. FP64 throughout; every
// product, quotient, sum and difference is rounded on its own (-ffp-contract=off); no libm call.
#pragma once
#include "occupancy_math.h"

namespace loamx {

enum { kRayClear = 0, kRayHit = 1, kRayUnknown = 2, kRayTruncated = 3, kRayOutside = 4, kRayInvalid = 5, kRayStatuses = 6 };  // LOAMX_RAY_*
enum { kRayAtEnter = 0, kRayAtMiddle = 1 };                                                                                  // LOAMX_RAY_AT_*
constexpr uint32_t kRayDefaultMaxSteps = 3u * 4098u;  // the bound of a walk of the map's own add
constexpr uint32_t kRayMaxSteps = 1u << 22;

struct RayRule {  // loamx_raycast_params
  uint32_t skip_start, unknown_stops, max_steps, hit_at;
};
struct RayRecord {  // loamx_ray_record
  uint32_t status, visits;
  int32_t voxel[3];
  uint32_t n_unknown;
  double t_enter, t_exit;
};

// occ_walk_step with the picked t_max, before it is advanced, returned: the parameter at which the segment enters the voxel the
// step leads into. The same pick, the same ties. Only with steps left.
LOAMX_HD double ray_walk_step(OccWalk& w) {
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
  return best;
}

// the parameter at which the segment leaves the voxel the walk stands in: the smallest t_max among the axes with steps left, 1.0
// in the walk's last voxel
LOAMX_HD double ray_t_exit(const OccWalk& w) {
  bool any = false;
  double best = 1.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int a = 0; a < 3; a++)
    if (w.rem[a] > 0 && (!any || w.t_max[a] < best)) any = true, best = w.t_max[a];
  return best;
}

// One ray on its way. While `live` it stands in a voxel it has not dealt with yet: visit number `visits`, entered at t_enter.
struct RayCast {
  OccWalk w;
  uint32_t left;  // steps the walk has left
  uint32_t cap;   // steps the cap still allows
  uint32_t visits, n_unknown, status;
  double t_enter;
  bool live;
};

// a ray that stands nowhere and visits nothing, with the status given: a lane without a ray, a beam of a pose that is not finite
LOAMX_HD void ray_idle(RayCast& r, uint32_t status) {
  r.w = OccWalk{};
  r.left = r.cap = r.visits = r.n_unknown = 0u, r.status = status, r.t_enter = 0.0, r.live = false;
}

// validity and walk set-up: INVALID and OUTSIDE end here (live stays false), every other ray stands in visit 0
LOAMX_HD void ray_begin(Vec3 o, Vec3 e, double leaf, const RayRule& P, RayCast& r) {
  ray_idle(r, kRayClear);
  if (!(cloud_finite(o.x) && cloud_finite(o.y) && cloud_finite(o.z) && cloud_finite(e.x) && cloud_finite(e.y) && cloud_finite(e.z))) {
    r.status = kRayInvalid;
    return;
  }
  if (!occ_walk_begin(o, e, leaf, r.w)) {
    r.status = kRayOutside;
    return;
  }
  r.left = occ_walk_steps(r.w), r.cap = P.max_steps, r.live = true;
}

// is the count word of the voxel the ray stands in wanted?
LOAMX_HD bool ray_tests(const RayCast& r, const RayRule& P) { return r.live && r.visits >= P.skip_start; }

// the visit of the voxel the ray stands in; `word` is its count word (hits << 32 | passes, 0 without a slot), looked at only where
// ray_tests. The ray stops here (live = false, status set) or steps into the next voxel.
LOAMX_HD void ray_visit(RayCast& r, unsigned long long word, const OccStateRule& sr, const RayRule& P) {
  const bool tested = r.visits >= P.skip_start;
  r.visits += 1u;
  if (tested) {
    const uint32_t st = occ_state((uint32_t)(word >> 32), (uint32_t)word, sr);
    if (st == kOccOccupied) {
      r.status = kRayHit, r.live = false;
      return;
    }
    if (st == kOccUnknown) {
      if (P.unknown_stops) {
        r.status = kRayUnknown, r.live = false;
        return;
      }
      r.n_unknown += 1u;
    }
  }
  if (r.left == 0u) {
    r.status = kRayClear, r.live = false;
    return;
  }
  if (r.cap == 0u) {
    r.status = kRayTruncated, r.live = false;
    return;
  }
  r.t_enter = ray_walk_step(r.w);
  r.left -= 1u, r.cap -= 1u;
}

// the record of a ray that has stopped
LOAMX_HD void ray_record(const RayCast& r, RayRecord& out) {
  out.status = r.status;
  if (r.status == kRayOutside || r.status == kRayInvalid) {
    out.visits = 0u, out.voxel[0] = out.voxel[1] = out.voxel[2] = 0, out.n_unknown = 0u, out.t_enter = 0.0, out.t_exit = 0.0;
    return;
  }
  out.visits = r.visits, out.n_unknown = r.n_unknown;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int a = 0; a < 3; a++) out.voxel[a] = (int32_t)r.w.b[a] - 1048576;
  out.t_enter = r.t_enter, out.t_exit = ray_t_exit(r.w);
}

// beam `d` (sensor frame) of a scan rendered at `pose` (7 doubles): false for a pose with an entry that is not finite (the beam
// is INVALID), otherwise the segment from the pose's translation to max_range along the beam
LOAMX_HD bool ray_beam(const double pose[7], Vec3 d, double max_range, Vec3& o, Vec3& e) {
  bool ok = true;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < 7; k++) ok = ok && cloud_finite(pose[k]);
  o = e = v3(0.0, 0.0, 0.0);
  if (!ok) return false;
  o = v3(pose[4], pose[5], pose[6]);
  e = pose_act(pose, v3(max_range * d.x, max_range * d.y, max_range * d.z));
  return true;
}

// the return of a rendered beam: range and point in the sensor frame; no HIT: range 0 and the point (+0, +0, +0)
LOAMX_HD void ray_return(const RayRecord& rec, Vec3 d, double max_range, uint32_t hit_at, double& range, Vec3& p) {
  range = 0.0, p = v3(0.0, 0.0, 0.0);
  if (rec.status != kRayHit) return;
  const double tau = hit_at == kRayAtEnter ? rec.t_enter : 0.5 * (rec.t_enter + rec.t_exit);
  range = tau * max_range;
  p = v3(range * d.x, range * d.y, range * d.z);
}

// one whole ray on the host or in one lane: `lookup(key)` gives the count word of a voxel. The kernels run the same functions with
// the lanes of a wavefront in step (raycast_kernels.hip).
template <typename Lookup>
LOAMX_HD void ray_cast(Vec3 o, Vec3 e, double leaf, const OccStateRule& sr, const RayRule& P, Lookup lookup, RayRecord& out) {
  RayCast r;
  ray_begin(o, e, leaf, P, r);
  while (r.live) ray_visit(r, ray_tests(r, P) ? lookup(occ_walk_key(r.w)) : 0ull, sr, P);
  ray_record(r, out);
}

}  // namespace loamx
