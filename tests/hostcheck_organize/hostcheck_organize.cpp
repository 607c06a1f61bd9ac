// TEST-ONLY: organize_math.h (the tables of a scan layout and the per-point classification of the organise kernels) compiled
// for the host behind extern "C" wrappers, for tests/test_organize_hostcheck.py. With -DHOSTCHECK_ORGANIZE_MAIN the file is a
// stand-alone program that runs the same wrappers over generated inputs and checks them against a plain scan of all W signs
// and all H + 1 comparisons (the `san` target builds it with -fsanitize=address,undefined).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../loam_amd/csrc/organize_math.h"

using namespace loamx;

extern "C" {

// col_dirs[W][2]; elevations == nullptr: linear from fov_bottom to fov_top. Returns 0, or 1 when the elevations are refused
// (fov_top <= fov_bottom with H > 1 included, as loamx_scan_layout_create does)
int hostcheck_organize_tables(double azimuth_zero, int clockwise, const double* elevations, double fov_bottom, double fov_top, uint32_t H, uint32_t W,
                              double* col_dirs, double* line_tans) {
  organize_column_dirs(azimuth_zero, clockwise != 0, W, col_dirs);
  std::vector<double> el(H, 0.0);
  if (elevations) {
    for (uint32_t i = 0; i < H; i++) el[i] = elevations[i];
  } else if (H > 1) {
    if (!(fov_top > fov_bottom)) return 1;
    for (uint32_t i = 0; i < H; i++) el[i] = organize_linear_elevation(fov_bottom, fov_top, H, i);
  }
  return organize_line_tans(el.data(), H, line_tans) ? 1 : 0;
}

// organize_cell of pts[i] (n x 3); rings: n ring numbers or nullptr; ring_map: n_ring_map entries or nullptr
void hostcheck_organize_cells(const double* col_dirs, const double* line_tans, uint32_t H, uint32_t W, int clockwise, const uint16_t* ring_map,
                              uint32_t n_ring_map, const double* pts, const uint16_t* rings, uint64_t n, uint32_t* cell, double* r2) {
  const OrgTables t{col_dirs, line_tans, ring_map, n_ring_map, H, W, clockwise ? 1u : 0u};
  for (uint64_t i = 0; i < n; i++) cell[i] = organize_cell(t, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], rings ? (uint32_t)rings[i] : kOrgNoRing, r2[i]);
}

}  // extern "C"

#ifdef HOSTCHECK_ORGANIZE_MAIN
#include <math.h>
int main() {
  uint64_t state = 88172645463325252ull;
  auto rnd = [&]() {
    state ^= state << 13, state ^= state >> 7, state ^= state << 17;
    return (double)(state >> 11) / 9007199254740992.0;
  };
  const uint32_t shapes[5][2] = {{1, 1}, {2, 2}, {8, 37}, {64, 1024}, {128, 4096}};
  uint64_t total = 0, placed = 0;
  for (int sh = 0; sh < 5; sh++) {
    const uint32_t H = shapes[sh][0], W = shapes[sh][1];
    for (int cw = 0; cw < 2; cw++) {
      std::vector<double> col(2 * (size_t)W), tans((size_t)H + 1);
      if (hostcheck_organize_tables(cw ? 0.3 : 0.0, cw, nullptr, -0.4, 0.2, H, W, col.data(), tans.data())) {
        printf("tables refused at %u x %u\n", H, W);
        return 1;
      }
      std::vector<double> pts;
      for (int i = 0; i < 4000; i++) pts.insert(pts.end(), {rnd() * 60.0 - 30.0, rnd() * 60.0 - 30.0, rnd() * 16.0 - 12.0});
      for (uint32_t k = 0; k < W; k += (W > 64 ? 61 : 1))  // on the boundaries, scaled by powers of two
        for (double rho : {0.25, 8.0}) pts.insert(pts.end(), {rho * col[2 * k], rho * col[2 * k + 1], rnd() - 0.5});
      for (uint32_t l = 0; l <= H; l++) pts.insert(pts.end(), {4.0, 0.0, 4.0 * tans[l]});
      pts.insert(pts.end(), {0.0, 0.0, 0.0, 0.0, 0.0, 3.0, NAN, 1.0, 2.0, 1.0, INFINITY, 2.0, 1.0, 2.0, -INFINITY, 1e-51, 0.0, 0.0, 1e-50, 1e-50, 0.0,
                             1e154, 1e154, 1e154, 1e150, -1e150, 1e149, 1e-49, 1e-49, -1e-49, -0.0, 2.0, -0.0});
      const uint64_t n = pts.size() / 3;
      std::vector<uint32_t> cell(n), cell_r(n);
      std::vector<double> r2(n);
      std::vector<uint16_t> rings(n), map(H + 2u);
      for (uint64_t i = 0; i < n; i++) rings[i] = (uint16_t)(rnd() * (H + 3));
      for (uint32_t i = 0; i < H + 2u; i++) map[i] = i < H ? (uint16_t)(H - 1 - i) : (uint16_t)0xFFFF;
      hostcheck_organize_cells(col.data(), tans.data(), H, W, cw, nullptr, 0, pts.data(), nullptr, n, cell.data(), r2.data());
      hostcheck_organize_cells(col.data(), tans.data(), H, W, cw, map.data(), H + 2u, pts.data(), rings.data(), n, cell_r.data(), r2.data());
      const OrgTables t{col.data(), tans.data(), nullptr, 0, H, W, (uint32_t)cw};
      for (uint64_t i = 0; i < n; i++) {
        const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        total++;
        if (cell[i] == kOrgCellInvalid) {
          if (cell_r[i] != kOrgCellInvalid) return printf("point %llu: invalid without rings only\n", (unsigned long long)i), 1;
          continue;
        }
        // the plain scans: every sign, every comparison
        uint32_t ncol = 0, c_ref = 0, cnt = 0;
        if (W > 1) {
          for (uint32_t k = 0; k < W; k++)
            if (organize_side(t, k, x, y) && !organize_side(t, k + 1 == W ? 0 : k + 1, x, y)) ncol++, c_ref = k;
        } else {
          ncol = 1;
        }
        const double rho = sqrt(x * x + y * y);
        for (uint32_t l = 0; l <= H; l++) cnt += z >= tans[l] * rho ? 1 : 0;
        if (ncol == 1) {
          const uint32_t want = (cnt == 0 || cnt == H + 1) ? kOrgCellOutside : (cnt - 1) * W + c_ref;
          if (cell[i] != want) return printf("%u x %u point %llu: cell %u, plain scan %u\n", H, W, (unsigned long long)i, cell[i], want), 1;
          const uint32_t line = rings[i] < H + 2u ? map[rings[i]] : 0xFFFFu;
          const uint32_t want_r = line == 0xFFFFu ? kOrgCellOutside : line * W + c_ref;
          if (cell_r[i] != want_r) return printf("%u x %u point %llu: ring cell %u, expected %u\n", H, W, (unsigned long long)i, cell_r[i], want_r), 1;
        } else if (W > 2) {
          return printf("%u x %u point %llu has %u columns\n", H, W, (unsigned long long)i, ncol), 1;
        }
        placed += cell[i] < kOrgCellInvalid ? 1 : 0;
      }
    }
  }
  if (placed == 0) return printf("no point was placed\n"), 1;
  printf("hostcheck_organize ok: %llu points, %llu placed\n", (unsigned long long)total, (unsigned long long)placed);
  return 0;
}
#endif
