// TEST-ONLY: distance_math.h (the rule of the occupancy distance field) compiled for the host as a program of its own, for
// tests/test_distance_hostcheck.py (the file formats: tests/distance_common.py).
//   hostcheck_distance IN OUT
// IN: cases back to back, each a header {dims[3], R, slice, early, n_obstacles, 0: uint32; leaf: double} and the obstacles as
// n_obstacles x 3 uint32 positions in the extended box (a slice: z = 0). OUT: per case d2 (uint16 [n]), offsets (int16 [n][3], a
// slice [n][2]), metres (float [n]). The passes run in the order and on the layouts of distance_kernels.hip: mask words, x, y, z.
// The `san` target builds the same file with -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../loam_amd/csrc/distance_math.h"

using namespace loamx;

struct Header {
  uint32_t dims[3], R, slice, early, n_obstacles, pad;
  double leaf;
};
static_assert(sizeof(Header) == 40, "the format of tests/distance_common.py");

struct CostDx {
  const int16_t* p;
  long long stride;
  uint32_t operator()(int32_t k) const { return dist_cost_dx((int32_t)p[k * stride]); }
};
struct CostDxy {
  const uint32_t* p;
  long long stride;
  uint32_t operator()(int32_t k) const { return dist_cost_dxy(p[k * stride]); }
};

static bool write_all(FILE* f, const void* p, size_t bytes) { return bytes == 0 || fwrite(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 1;
  }
  FILE* f = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!f || !out) {
    fprintf(stderr, "cannot open %s or %s\n", argv[1], argv[2]);
    return 2;
  }
  Header h;
  while (fread(&h, sizeof(h), 1, f) == 1) {
    const uint32_t R = h.R, dx = h.dims[0], dy = h.dims[1], dz = h.slice ? 1u : h.dims[2];
    const uint32_t ex = dx + 2 * R, ey = dy + 2 * R, ez = h.slice ? 1u : dz + 2 * R, W = (ex + 63) / 64;
    const size_t rows = (size_t)ey * ez;
    std::vector<uint32_t> obst((size_t)h.n_obstacles * 3);
    if (obst.size() && fread(obst.data(), sizeof(uint32_t), obst.size(), f) != obst.size()) {
      fprintf(stderr, "short obstacle list\n");
      return 3;
    }
    // mask words
    std::vector<unsigned long long> mask(rows * W, 0ull);
    for (size_t i = 0; i < h.n_obstacles; i++) {
      const uint32_t x = obst[3 * i], y = obst[3 * i + 1], z = obst[3 * i + 2];
      if (x >= ex || y >= ey || z >= ez) {
        fprintf(stderr, "obstacle outside the extended box\n");
        return 3;
      }
      mask[((size_t)z * ey + y) * W + (x >> 6)] |= 1ull << (x & 63);
    }
    // x-pass
    std::vector<int16_t> sx(rows * dx);
    for (size_t r = 0; r < rows; r++)
      for (uint32_t x = 0; x < dx; x++) sx[r * dx + x] = (int16_t)dist_x_pass(mask.data() + r * W, x + R, R);
    const size_t n = (size_t)dx * dy * dz, axes = h.slice ? 2 : 3;
    std::vector<uint16_t> d2(n);
    std::vector<int16_t> off(n * axes);
    std::vector<float> metres(n);
    // y-pass: a slab per level of the extended box
    std::vector<uint32_t> sxy((size_t)ez * dy * dx);
    std::vector<int32_t> ky(sxy.size());
    std::vector<uint32_t> cost_y(sxy.size());
    for (uint32_t o = 0; o < ez; o++)
      for (uint32_t r = 0; r < dy; r++)
        for (uint32_t j = 0; j < dx; j++) {
          const int16_t* p = sx.data() + ((size_t)o * ey + r + R) * dx + j;
          int32_t k = 0;
          const uint32_t best = dist_column_pass(CostDx{p, (long long)dx}, R, h.early != 0, k);
          const size_t i = ((size_t)o * dy + r) * dx + j;
          sxy[i] = best != kDistNone ? dist_pack((int32_t)p[(long long)k * dx], k) : kDistNoDxy;
          ky[i] = k, cost_y[i] = best;
        }
    if (h.slice) {
      for (size_t i = 0; i < n; i++) {
        const bool far = cost_y[i] == kDistNone, zero = far || cost_y[i] == 0;
        d2[i] = (uint16_t)(far ? kDistFar : cost_y[i]);
        off[2 * i] = (int16_t)(zero ? 0 : dist_dx(sxy[i])), off[2 * i + 1] = (int16_t)(zero ? 0 : ky[i]);
        metres[i] = dist_metres(d2[i], h.leaf);
      }
    } else {
      const size_t plane = (size_t)dx * dy;
      for (uint32_t r = 0; r < dz; r++)
        for (size_t j = 0; j < plane; j++) {
          const uint32_t* p = sxy.data() + ((size_t)r + R) * plane + j;
          int32_t k = 0;
          const uint32_t best = dist_column_pass(CostDxy{p, (long long)plane}, R, h.early != 0, k);
          const size_t i = (size_t)r * plane + j;
          const bool far = best == kDistNone, zero = far || best == 0;
          const uint32_t w = far ? kDistNoDxy : p[(long long)k * (long long)plane];
          d2[i] = (uint16_t)(far ? kDistFar : best);
          off[3 * i] = (int16_t)(zero ? 0 : dist_dx(w)), off[3 * i + 1] = (int16_t)(zero ? 0 : dist_dy(w)), off[3 * i + 2] = (int16_t)(zero ? 0 : k);
          metres[i] = dist_metres(d2[i], h.leaf);
        }
    }
    if (!write_all(out, d2.data(), n * sizeof(uint16_t)) || !write_all(out, off.data(), n * axes * sizeof(int16_t)) ||
        !write_all(out, metres.data(), n * sizeof(float))) {
      fprintf(stderr, "cannot write %s\n", argv[2]);
      return 4;
    }
  }
  fclose(f);
  if (fclose(out) != 0) return 4;
  return 0;
}
