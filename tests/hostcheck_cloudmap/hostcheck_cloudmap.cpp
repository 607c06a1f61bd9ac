// TEST-ONLY: cloudmap_math.h (the per-point arithmetic of the cloud map kernels) compiled for the host behind extern "C"
// wrappers, for tests/test_cloudmap_hostcheck.py. With -DHOSTCHECK_CLOUDMAP_MAIN the file is a stand-alone program that folds
// generated points into a std::map table with the same functions (the `san` target builds it with -fsanitize=address,undefined).
#include <stdint.h>
#include <stdio.h>

#include <map>
#include <vector>

#include "../../loam_amd/csrc/cloudmap_math.h"

using namespace loamx;

extern "C" {

// what[i]: kCloud* of pts[i] (n x 3) by the range test alone
void hostcheck_cloudmap_validity(const double* pts, uint64_t n, double min_r2, double max_r2, int32_t* what) {
  for (uint64_t i = 0; i < n; i++) what[i] = cloud_validity(v3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]), min_r2, max_r2);
}

// keys[i], u[i][3] of pts[i] at `leaf`; ok[i] = 0 where the point has no voxel
void hostcheck_cloudmap_cells(const double* pts, uint64_t n, double leaf, uint64_t* keys, uint32_t* u, uint8_t* ok) {
  for (uint64_t i = 0; i < n; i++) {
    uint64_t key = 0;
    ok[i] = cloud_cell(v3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]), leaf, key, u + 3 * i) ? 1 : 0;
    keys[i] = key;
  }
}

// out[i][a] = centroid of voxel keys[i] with sums[i][a] and counts[i]
void hostcheck_cloudmap_centroids(const uint64_t* keys, const uint64_t* sums, const uint32_t* counts, uint64_t n, double leaf, double* out) {
  for (uint64_t i = 0; i < n; i++)
    for (int a = 0; a < 3; a++) out[3 * i + a] = cloud_centroid(cloud_key_coord(keys[i], a), sums[3 * i + a], counts[i], leaf);
}

}  // extern "C"

#ifdef HOSTCHECK_CLOUDMAP_MAIN
#include <math.h>
struct Voxel {
  uint64_t sum[3] = {0, 0, 0};
  uint32_t count = 0, first = 0xFFFFFFFFu;
};
int main() {
  // voxel faces, random points, the clamp, the range edges and non-finite values
  std::vector<double> pts;
  uint64_t state = 88172645463325252ull;
  auto rnd = [&]() {
    state ^= state << 13, state ^= state >> 7, state ^= state << 17;
    return (double)(state >> 11) / 9007199254740992.0;
  };
  for (int i = -50; i < 50; i++) pts.insert(pts.end(), {i * 0.4, -i * 0.4, 1.0});
  for (int i = 0; i < 6000; i++) pts.insert(pts.end(), {rnd() * 40.0 - 20.0, rnd() * 40.0 - 20.0, rnd() * 4.0 - 2.0});
  const double edge = 1048576.0 * 0.4;
  pts.insert(pts.end(), {edge, -edge, nextafter(edge, 0.0), -0.0, 1.0, -1e-20, 1e-20, -1e-20, 1.0, NAN, INFINITY, -INFINITY, 1e300, -1e300, 1e9,
                         0.0, 0.0, 0.0, 1e200, 1.0, 1.0});
  const uint64_t n = pts.size() / 3;
  const double leaf = 0.4, min_r2 = 0.25, max_r2 = 1e12;
  std::vector<int32_t> what(n);
  std::vector<uint64_t> keys(n);
  std::vector<uint32_t> u(3 * n);
  std::vector<uint8_t> ok(n);
  hostcheck_cloudmap_validity(pts.data(), n, min_r2, max_r2, what.data());
  hostcheck_cloudmap_cells(pts.data(), n, leaf, keys.data(), u.data(), ok.data());
  std::map<uint64_t, Voxel> table;
  uint64_t used = 0, clamped = 0;
  for (uint64_t i = 0; i < n; i++) {
    if (what[i] != kCloudUsed || !ok[i]) continue;
    Voxel& v = table[keys[i]];
    for (int a = 0; a < 3; a++) v.sum[a] += u[3 * i + a], clamped += u[3 * i + a] == 0xFFFFFFFFu;
    v.count++, used++;
    if ((uint32_t)i < v.first) v.first = (uint32_t)i;
  }
  std::vector<uint64_t> k2, s2;
  std::vector<uint32_t> c2;
  for (const auto& kv : table) {
    k2.push_back(kv.first), c2.push_back(kv.second.count);
    s2.insert(s2.end(), kv.second.sum, kv.second.sum + 3);
  }
  std::vector<double> cen(3 * k2.size());
  hostcheck_cloudmap_centroids(k2.data(), s2.data(), c2.data(), k2.size(), leaf, cen.data());
  for (size_t j = 0; j < k2.size(); j++)
    for (int a = 0; a < 3; a++) {
      const double lo = (double)cloud_key_coord(k2[j], a) * leaf, c = cen[3 * j + a];
      if (!(c >= lo - 1e-9 && c <= lo + leaf + 1e-9)) {
        printf("centroid %g outside its voxel [%g, %g]\n", c, lo, lo + leaf);
        return 1;
      }
    }
  if (!clamped || used == 0 || used == n) {
    printf("the inputs no longer reach the clamp, or nothing / everything was used\n");
    return 1;
  }
  printf("hostcheck_cloudmap ok: %llu points, %llu used, %llu voxels, %llu clamped offsets\n", (unsigned long long)n, (unsigned long long)used,
         (unsigned long long)table.size(), (unsigned long long)clamped);
  return 0;
}
#endif
