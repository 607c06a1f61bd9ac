// TEST-ONLY: raycast_math.h (the per-ray arithmetic of the ray cast kernels) compiled for the host behind extern "C" wrappers, for
// tests/test_raycast_hostcheck.py. The map is a sorted array of keys with their count words. With -DHOSTCHECK_RAYCAST_MAIN the file
// is a stand-alone program that casts generated rays with the same functions (the `san` target builds it with
// -fsanitize=address,undefined).
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../loam_amd/csrc/raycast_math.h"

using namespace loamx;

namespace {

struct Table {
  const uint64_t* keys;  // ascending
  const uint64_t* words;
  uint64_t n;
  unsigned long long operator()(uint64_t key) const {
    const uint64_t* it = std::lower_bound(keys, keys + n, key);
    return it != keys + n && *it == key ? words[it - keys] : 0ull;
  }
};

OccStateRule state_rule(uint32_t min_hits, double occ_ratio, uint32_t min_passes) {
  OccStateRule s;
  s.min_hits = min_hits, s.min_passes = min_passes, s.occ_ratio = occ_ratio;
  return s;
}

}  // namespace

static_assert(sizeof(RayRecord) == 40, "a ray record is 40 bytes");

extern "C" {

// params: skip_start, unknown_stops, max_steps, hit_at
void hostcheck_raycast_cast(const double* origins, const double* ends, uint64_t n, double leaf, const uint64_t* keys, const uint64_t* words,
                            uint64_t n_vox, uint32_t min_hits, double occ_ratio, uint32_t min_passes, const uint32_t* params, RayRecord* out) {
  const Table t = {keys, words, n_vox};
  const OccStateRule sr = state_rule(min_hits, occ_ratio, min_passes);
  const RayRule P = {params[0], params[1], params[2], params[3]};
  for (uint64_t i = 0; i < n; i++)
    ray_cast(v3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]), v3(ends[3 * i], ends[3 * i + 1], ends[3 * i + 2]), leaf, sr, P, t, out[i]);
}

void hostcheck_raycast_render(const double* dirs, uint64_t n_beams, const double* poses, uint64_t n_poses, double max_range, double leaf,
                              const uint64_t* keys, const uint64_t* words, uint64_t n_vox, uint32_t min_hits, double occ_ratio, uint32_t min_passes,
                              const uint32_t* params, double* scans, double* ranges, RayRecord* out) {
  const Table t = {keys, words, n_vox};
  const OccStateRule sr = state_rule(min_hits, occ_ratio, min_passes);
  const RayRule P = {params[0], params[1], params[2], params[3]};
  for (uint64_t p = 0; p < n_poses; p++)
    for (uint64_t b = 0; b < n_beams; b++) {
      const uint64_t i = p * n_beams + b;
      const Vec3 d = v3(dirs[3 * b], dirs[3 * b + 1], dirs[3 * b + 2]);
      Vec3 o, e;
      if (ray_beam(poses + 7 * p, d, max_range, o, e)) {
        ray_cast(o, e, leaf, sr, P, t, out[i]);
      } else {
        RayCast r;
        ray_idle(r, kRayInvalid);
        ray_record(r, out[i]);
      }
      Vec3 pt;
      ray_return(out[i], d, max_range, P.hit_at, ranges[i], pt);
      scans[3 * i] = pt.x, scans[3 * i + 1] = pt.y, scans[3 * i + 2] = pt.z;
    }
}

// every visit of one walk that begins (the map plays no part): key, t_enter and t_exit, at most `room` of them; returns the number
// of visits of the whole walk, 0 for a segment that is not finite or leaves the voxel range
uint32_t hostcheck_raycast_visits(const double* o, const double* e, double leaf, uint32_t room, uint64_t* keys, double* t_enter, double* t_exit) {
  const RayRule P = {0u, 0u, kRayMaxSteps, kRayAtMiddle};
  RayCast r;
  ray_begin(v3(o[0], o[1], o[2]), v3(e[0], e[1], e[2]), leaf, P, r);
  if (!r.live) return 0u;
  const uint32_t steps = occ_walk_steps(r.w);
  double enter = 0.0;
  for (uint32_t k = 0; k <= steps; k++) {
    if (k < room) keys[k] = occ_walk_key(r.w), t_enter[k] = enter, t_exit[k] = ray_t_exit(r.w);
    if (k < steps) enter = ray_walk_step(r.w);
  }
  return steps + 1u;
}

}  // extern "C"

#ifdef HOSTCHECK_RAYCAST_MAIN
#include <math.h>
int main() {
  uint64_t state = 88172645463325252ull;
  auto rnd = [&]() {
    state ^= state << 13, state ^= state >> 7, state ^= state << 17;
    return (double)(state >> 11) / 9007199254740992.0;
  };
  // a random map inside +-10 m at leaf 0.4
  const double leaf = 0.4;
  std::vector<std::pair<uint64_t, uint64_t>> vox;
  for (int i = 0; i < 3000; i++) {
    uint64_t key;
    uint32_t u[3];
    if (cloud_cell(v3(rnd() * 20.0 - 10.0, rnd() * 20.0 - 10.0, rnd() * 4.0 - 2.0), leaf, key, u))
      vox.push_back({key, (uint64_t)(rnd() * 3.0) << 32 | (uint64_t)(rnd() * 4.0)});
  }
  std::sort(vox.begin(), vox.end());
  vox.erase(std::unique(vox.begin(), vox.end(), [](const auto& a, const auto& b) { return a.first == b.first; }), vox.end());
  std::vector<uint64_t> keys, words;
  for (const auto& kv : vox) keys.push_back(kv.first), words.push_back(kv.second);
  // random segments, lattice corners, zero-length, far, outside and non-finite ones
  std::vector<double> o, e;
  for (int i = 0; i < 4000; i++) {
    o.insert(o.end(), {rnd() * 24.0 - 12.0, rnd() * 24.0 - 12.0, rnd() * 6.0 - 3.0});
    e.insert(e.end(), {rnd() * 24.0 - 12.0, rnd() * 24.0 - 12.0, rnd() * 6.0 - 3.0});
  }
  for (int i = 1; i < 30; i++) {
    o.insert(o.end(), {0.0, 0.0, 0.0, i * 0.4, 0.0, -0.0, i * 0.4, i * 0.4, i * 0.4});
    e.insert(e.end(), {i * 0.4, i * 0.4, i * 0.4, -i * 0.4, -i * 0.4, 0.0, i * 0.4, i * 0.4, i * 0.4});
  }
  o.insert(o.end(), {NAN, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1e300, 0.0, 0.0});
  e.insert(e.end(), {1.0, 0.0, 0.0, INFINITY, 1.0, 1.0, 5e5, 0.0, 0.0, 2000.0, 1500.0, -300.0, 0.0, 0.0, 0.0});
  const uint64_t n = o.size() / 3;
  uint64_t by_status[kRayStatuses] = {}, visits = 0;
  const uint32_t variants[5][4] = {{0, 0, kRayDefaultMaxSteps, 1}, {1, 1, kRayDefaultMaxSteps, 0}, {0, 0, 5, 1}, {3, 0, 0, 1}, {0, 1, kRayMaxSteps, 1}};
  for (const auto& P : variants) {
    std::vector<RayRecord> rec(n);
    hostcheck_raycast_cast(o.data(), e.data(), n, leaf, keys.data(), words.data(), keys.size(), 1, 0.25, 1, P, rec.data());
    for (const RayRecord& r : rec) {
      by_status[r.status]++, visits += r.visits;
      if (r.status > kRayInvalid || r.visits > (uint64_t)P[2] + 1u || !(r.t_enter <= r.t_exit) || !(r.t_exit <= 1.0 + 1e-9)) {
        printf("a record breaks the rule: status %u visits %u t %g %g\n", r.status, r.visits, r.t_enter, r.t_exit);
        return 1;
      }
    }
    // the same rays as the beams of two poses, one of them not finite
    std::vector<double> dirs;
    for (int i = 0; i < 200; i++) {
      const double x = rnd() - 0.5, y = rnd() - 0.5, z = 0.2 * (rnd() - 0.5), s = 1.0 / sqrt(x * x + y * y + z * z);
      dirs.insert(dirs.end(), {x * s, y * s, z * s});
    }
    const double poses[3][7] = {{0.0, 0.0, 0.3826834323650898, 0.9238795325112867, 1.3, -2.1, 0.4}, {0, 0, 0, 1, 0, NAN, 0}, {0, 0, 0, 1, 0.0, 0.0, 0.0}};
    std::vector<double> scans(3 * 200 * 3), ranges(3 * 200);
    std::vector<RayRecord> rrec(3 * 200);
    hostcheck_raycast_render(dirs.data(), 200, &poses[0][0], 3, 15.0, leaf, keys.data(), words.data(), keys.size(), 1, 0.25, 1, P, scans.data(),
                             ranges.data(), rrec.data());
    for (int i = 0; i < 600; i++) {
      by_status[rrec[i].status]++;
      if ((rrec[i].status == kRayHit) != (ranges[i] > 0.0 || (rrec[i].status == kRayHit && rrec[i].t_enter == 0.0)) || (i / 200 == 1) != (rrec[i].status == kRayInvalid)) {
        printf("a rendered beam breaks the rule: %d status %u range %g\n", i, rrec[i].status, ranges[i]);
        return 1;
      }
    }
  }
  // every visit of a long diagonal walk, written into exactly the room given
  {
    const double a[3] = {-11.3, 7.1, -2.9}, b[3] = {12.2, -9.4, 2.2};
    const uint32_t total = hostcheck_raycast_visits(a, b, leaf, 0, nullptr, nullptr, nullptr);
    std::vector<uint64_t> k(total);
    std::vector<double> t0(total), t1(total);
    if (hostcheck_raycast_visits(a, b, leaf, total, k.data(), t0.data(), t1.data()) != total) return 1;
    for (uint32_t v = 0; v + 1 < total; v++)
      if (t1[v] != t0[v + 1] || !(t0[v] <= t1[v])) {
        printf("visit %u: t_exit %g, next t_enter %g\n", v, t1[v], t0[v + 1]);
        return 1;
      }
  }
  for (int s = 0; s < kRayStatuses; s++)
    if (!by_status[s]) {
      printf("the inputs no longer reach status %d\n", s);
      return 1;
    }
  printf("hostcheck_raycast ok: %llu rays x 5, %llu visits\n", (unsigned long long)n, (unsigned long long)visits);
  return 0;
}
#endif
