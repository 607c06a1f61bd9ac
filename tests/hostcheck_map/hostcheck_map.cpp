// TEST-ONLY: map_math.h (the per-point arithmetic of the map upkeep kernels) compiled for the host behind extern "C"
// wrappers, for tests/test_map_hostcheck.py. With -DHOSTCHECK_MAP_MAIN the file is a stand-alone program that runs the
// same wrappers over generated inputs (the `san` target builds it with -fsanitize=address,undefined).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../loam_amd/csrc/map_math.h"

using namespace loamx;

extern "C" {

// keys[i] of pts[i] (n x 3) at `leaf`, ok[i] = 0 where the point has no voxel (non-finite or out of range)
void hostcheck_map_keys(const double* pts, uint64_t n, double leaf, uint64_t* keys, uint8_t* ok) {
  for (uint64_t i = 0; i < n; i++) {
    uint64_t key = 0;
    ok[i] = voxel_key(v3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]), leaf, key) ? 1 : 0;
    keys[i] = key;
  }
}

// largest slot voxel_hash gives over the keys at this capacity, and the OR of all slots (a hash stuck in a few bits shows)
void hostcheck_map_hash_range(const uint64_t* keys, uint64_t n, uint32_t log2_cap, uint32_t* max_slot, uint32_t* or_slots) {
  uint32_t mx = 0, acc = 0;
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t s = voxel_hash(keys[i], log2_cap);
    mx = s > mx ? s : mx, acc |= s;
  }
  *max_slot = mx, *or_slots = acc;
}

void hostcheck_map_pose_act(const double* pose, const double* pts, uint64_t n, double* out) {
  for (uint64_t i = 0; i < n; i++) {
    const Vec3 p = pose_act(pose, v3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]));
    out[3 * i] = p.x, out[3 * i + 1] = p.y, out[3 * i + 2] = p.z;
  }
}

int hostcheck_map_pose_is_identity(const double* pose) { return pose_is_identity(pose) ? 1 : 0; }

void hostcheck_map_box(const double* pts, uint64_t n, const double* lo, const double* hi, uint8_t* inside) {
  for (uint64_t i = 0; i < n; i++) inside[i] = box_holds(v3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]), lo, hi) ? 1 : 0;
}

}  // extern "C"

#ifdef HOSTCHECK_MAP_MAIN
#include <math.h>
int main() {
  // a lattice of leaf multiples, random points, the range edges and non-finite values
  std::vector<double> pts;
  uint64_t state = 88172645463325252ull;
  auto rnd = [&]() {
    state ^= state << 13, state ^= state >> 7, state ^= state << 17;
    return (double)(state >> 11) / 9007199254740992.0;
  };
  for (int i = -50; i < 50; i++) pts.insert(pts.end(), {i * 0.4, -i * 0.4, 0.0});
  for (int i = 0; i < 100000; i++) pts.insert(pts.end(), {rnd() * 200.0 - 100.0, rnd() * 200.0 - 100.0, rnd() * 20.0 - 10.0});
  const double edge = 1048576.0 * 0.4;
  pts.insert(pts.end(), {edge, -edge, nextafter(edge, 0.0), -0.0, 0.0, nextafter(-edge, 0.0), NAN, INFINITY, -INFINITY, 1e300, -1e300, 1e9});
  const uint64_t n = pts.size() / 3;
  std::vector<uint64_t> keys(n);
  std::vector<uint8_t> ok(n), inside(n);
  hostcheck_map_keys(pts.data(), n, 0.4, keys.data(), ok.data());
  uint64_t n_ok = 0;
  for (uint64_t i = 0; i < n; i++) n_ok += ok[i];
  for (uint32_t l = 4; l <= 24; l++) {
    uint32_t mx = 0, acc = 0;
    hostcheck_map_hash_range(keys.data(), n, l, &mx, &acc);
    if (mx >= (1u << l)) {
      printf("hash outside the table at capacity 2^%u\n", l);
      return 1;
    }
  }
  const double pose[7] = {0.01, -0.02, 0.03, 0.999, 1.0, 2.0, 3.0}, ident[7] = {0, 0, 0, 1, 0, 0, 0};
  std::vector<double> moved(pts.size());
  hostcheck_map_pose_act(pose, pts.data(), n, moved.data());
  const double lo[3] = {-10.0, -INFINITY, -1.0}, hi[3] = {10.0, INFINITY, 1.0};
  hostcheck_map_box(moved.data(), n, lo, hi, inside.data());
  if (!hostcheck_map_pose_is_identity(ident) || hostcheck_map_pose_is_identity(pose)) return 1;
  printf("hostcheck_map ok: %llu points, %llu with a voxel\n", (unsigned long long)n, (unsigned long long)n_ok);
  return 0;
}
#endif
