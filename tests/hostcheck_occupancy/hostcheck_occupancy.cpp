// TEST-ONLY: occupancy_math.h (the per-ray arithmetic of the occupancy map kernels) compiled for the host behind extern "C"
// wrappers, for tests/test_occupancy_hostcheck.py. With -DHOSTCHECK_OCCUPANCY_MAIN the file is a stand-alone program that walks
// generated rays into a std::map table with the same functions (the `san` target builds it with -fsanitize=address,undefined).
#include <stdint.h>
#include <stdio.h>

#include <map>
#include <set>
#include <vector>

#include "../../loam_amd/csrc/occupancy_math.h"

using namespace loamx;

static OccRule make_rule(double leaf, double min_range, double max_range, double end_margin, uint32_t clip_long) {
  OccRule R;
  R.leaf = leaf, R.min_r2 = min_range * min_range, R.max_r2 = max_range * max_range;
  R.max_range = max_range, R.end_margin = end_margin, R.clip_long = clip_long;
  return R;
}

static void one_ray(const double* pts, uint64_t i, const double* pose, const OccRule& R, OccRay& r) {
  const double ident[7] = {0, 0, 0, 1, 0, 0, 0};
  occ_ray(v3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]), pose != nullptr, pose ? pose : ident, R, r);
}

extern "C" {

// per ray of pts (n x 3) at `pose` (7 doubles or null): kind[i] = kOccRay*, flags[i] = has_hit | outside << 1 | walks << 2,
// hit_key[i] (0 without a hit), steps[i] = the steps of its walk (0 without one)
void hostcheck_occupancy_rays(const double* pts, uint64_t n, const double* pose, double leaf, double min_range, double max_range, double end_margin,
                              uint32_t clip_long, int32_t* kind, uint8_t* flags, uint64_t* hit_key, uint32_t* steps) {
  const OccRule R = make_rule(leaf, min_range, max_range, end_margin, clip_long);
  for (uint64_t i = 0; i < n; i++) {
    OccRay r;
    one_ray(pts, i, pose, R, r);
    kind[i] = r.kind, flags[i] = (uint8_t)((r.has_hit ? 1 : 0) | (r.outside ? 2 : 0) | (r.walks ? 4 : 0));
    hit_key[i] = r.has_hit ? r.hit_key : 0, steps[i] = r.walks ? occ_walk_steps(r.w) : 0;
  }
}

// the keys of every walking ray's voxels in order, ray i's at keys[first[i] ..]: steps[i] + 1 of them (first and steps as the
// caller has them from hostcheck_occupancy_rays)
void hostcheck_occupancy_walks(const double* pts, uint64_t n, const double* pose, double leaf, double min_range, double max_range, double end_margin,
                               uint32_t clip_long, const uint64_t* first, uint64_t* keys) {
  const OccRule R = make_rule(leaf, min_range, max_range, end_margin, clip_long);
  for (uint64_t i = 0; i < n; i++) {
    OccRay r;
    one_ray(pts, i, pose, R, r);
    if (!r.walks) continue;
    uint64_t* out = keys + first[i];
    const uint32_t steps = occ_walk_steps(r.w);
    *out++ = occ_walk_key(r.w);
    for (uint32_t s = 0; s < steps; s++) occ_walk_step(r.w), *out++ = occ_walk_key(r.w);
  }
}

void hostcheck_occupancy_states(const uint32_t* hits, const uint32_t* passes, uint64_t n, uint32_t min_hits, double occ_ratio, uint32_t min_passes,
                                uint8_t* out) {
  OccStateRule s;
  s.min_hits = min_hits, s.min_passes = min_passes, s.occ_ratio = occ_ratio;
  for (uint64_t i = 0; i < n; i++) out[i] = (uint8_t)occ_state(hits[i], passes[i], s);
}

}  // extern "C"

#ifdef HOSTCHECK_OCCUPANCY_MAIN
#include <math.h>
struct Counts {
  uint32_t hits = 0, passes = 0;
};
int main() {
  // random rays, axis-parallel and diagonal rays from lattice corners, faces, both range edges, long rays and non-finite values
  std::vector<double> pts;
  uint64_t state = 88172645463325252ull;
  auto rnd = [&]() {
    state ^= state << 13, state ^= state >> 7, state ^= state << 17;
    return (double)(state >> 11) / 9007199254740992.0;
  };
  for (int i = 0; i < 4000; i++) pts.insert(pts.end(), {rnd() * 60.0 - 30.0, rnd() * 60.0 - 30.0, rnd() * 6.0 - 3.0});
  for (int i = 1; i < 40; i++)
    pts.insert(pts.end(), {i * 0.4, 0.0, 0.0, 0.0, -i * 0.4, 0.0, i * 0.4, i * 0.4, 0.0, i * 0.4, i * 0.4, i * 0.4, -i * 0.4, -i * 0.4, i * 0.4});
  pts.insert(pts.end(), {NAN, 0.0, 0.0, INFINITY, 1.0, 1.0, 1e300, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5, 0.0, 0.0, nextafter(0.5, 0.0), 0.0, 0.0, 200.0, 3.0, 1.0,
                         -1e-20, 1.0, -0.0, 0.6, 1e-20, -1e-20, 5e5, 1.0, 1.0, 40.0, 0.0, 0.0, nextafter(40.0, 50.0), 0.0, 0.0});
  const uint64_t n = pts.size() / 3;
  const double poses[3][7] = {{0, 0, 0, 1, 0, 0, 0}, {0.0, 0.0, 0.3826834323650898, 0.9238795325112867, 1.3, -2.1, 0.4}, {0, 0, 0, 1, 419430.0, 0, 0}};
  uint64_t walked = 0, visited = 0, outside = 0, longs = 0;
  for (int clip = 0; clip < 2; clip++)
    for (int pi = -1; pi < 3; pi++) {
      const double* pose = pi < 0 ? nullptr : poses[pi];
      std::vector<int32_t> kind(n);
      std::vector<uint8_t> flags(n);
      std::vector<uint64_t> hit_key(n), first(n);
      std::vector<uint32_t> steps(n);
      hostcheck_occupancy_rays(pts.data(), n, pose, 0.4, 0.5, 40.0, 0.2, (uint32_t)clip, kind.data(), flags.data(), hit_key.data(), steps.data());
      uint64_t total = 0;
      for (uint64_t i = 0; i < n; i++) first[i] = total, total += (flags[i] & 4) ? steps[i] + 1 : 0;
      std::vector<uint64_t> keys(total);
      hostcheck_occupancy_walks(pts.data(), n, pose, 0.4, 0.5, 40.0, 0.2, (uint32_t)clip, first.data(), keys.data());
      std::map<uint64_t, Counts> table;
      for (uint64_t i = 0; i < n; i++) {
        outside += (flags[i] >> 1) & 1, longs += kind[i] == kOccRayLong;
        if (flags[i] & 1) table[hit_key[i]].hits++;
        if (!(flags[i] & 4)) continue;
        walked++;
        std::set<uint64_t> seen;
        for (uint64_t j = first[i]; j < first[i] + steps[i] + 1; j++) {
          if (!seen.insert(keys[j]).second) {
            printf("ray %llu visits a voxel twice\n", (unsigned long long)i);
            return 1;
          }
          if (!((flags[i] & 1) && keys[j] == hit_key[i])) table[keys[j]].passes++, visited++;
        }
        if (steps[i] > 3 * 4098) {
          printf("ray %llu takes %u steps\n", (unsigned long long)i, steps[i]);
          return 1;
        }
      }
      std::vector<uint32_t> h, p;
      for (const auto& kv : table) h.push_back(kv.second.hits), p.push_back(kv.second.passes);
      std::vector<uint8_t> st(h.size());
      hostcheck_occupancy_states(h.data(), p.data(), h.size(), 1, 0.5, 1, st.data());
      for (size_t j = 0; j < st.size(); j++)
        if (st[j] == kOccUnknown) {
          printf("a voxel of the table is unknown\n");
          return 1;
        }
    }
  if (!walked || !outside || !longs || visited < 10 * walked) {
    printf("the inputs no longer reach a walk, an outside ray or a long ray\n");
    return 1;
  }
  printf("hostcheck_occupancy ok: %llu rays x 8, %llu walks, %llu passes\n", (unsigned long long)n, (unsigned long long)walked, (unsigned long long)visited);
  return 0;
}
#endif
