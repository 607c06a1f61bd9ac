// TEST-ONLY: place_math.h (the per-point classification of a scan descriptor, the quantised cosine of two columns, the distance
// of a shift) compiled for the host behind extern "C" wrappers, for tests/test_place_hostcheck.py. With -DHOSTCHECK_PLACE_MAIN
// the file is a stand-alone program that runs the same wrappers over generated inputs and checks them against a plain scan of
// all S signs and a descriptor comparison written out shift by shift (the `san` target builds it with
// -fsanitize=address,undefined).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../loam_amd/csrc/place_math.h"

using namespace loamx;

extern "C" {

void hostcheck_place_dirs(uint32_t S, double* dirs) { organize_column_dirs(0.0, false, S, dirs); }

// place_cell of pts[i] (n x 3): cell[i] (kPlaceNoCell: dropped) and code[i]
void hostcheck_place_cells(uint32_t R, uint32_t S, double max_range, double z_offset, double z_scale, const double* dirs, const double* pts, uint64_t n,
                           uint32_t* cell, uint32_t* code) {
  const PlaceShape p{R, S, (double)R / max_range, z_offset, z_scale};
  for (uint64_t i = 0; i < n; i++) {
    code[i] = 0;
    cell[i] = place_cell(p, dirs, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], code[i]);
  }
}

void hostcheck_place_cos(const uint64_t* dot, const uint64_t* nq, const uint64_t* ne, uint64_t n, uint64_t* k) {
  for (uint64_t i = 0; i < n; i++) k[i] = place_cos_q(dot[i], nq[i], ne[i]);
}

void hostcheck_place_shift_distance(const uint64_t* score, const uint32_t* m, uint64_t n, double* dist) {
  for (uint64_t i = 0; i < n; i++) dist[i] = place_shift_distance(score[i], m[i]);
}

// q, e: R x S descriptors -> dist[S] over the shifts, from exact integer dots and norms; returns the best shift
uint32_t hostcheck_place_pair(const uint16_t* q, const uint16_t* e, uint32_t R, uint32_t S, double* dist) {
  std::vector<uint64_t> nq(S, 0), ne(S, 0);
  for (uint32_t r = 0; r < R; r++)
    for (uint32_t j = 0; j < S; j++) nq[j] += (uint64_t)q[r * S + j] * q[r * S + j], ne[j] += (uint64_t)e[r * S + j] * e[r * S + j];
  uint32_t best = 0;
  for (uint32_t s = 0; s < S; s++) {
    uint64_t score = 0;
    uint32_t m = 0;
    for (uint32_t j = 0; j < S; j++) {
      const uint32_t jj = (j + s) % S;
      if (!nq[j] || !ne[jj]) continue;
      uint64_t dot = 0;
      for (uint32_t r = 0; r < R; r++) dot += (uint64_t)q[r * S + j] * e[r * S + jj];
      score += place_cos_q(dot, nq[j], ne[jj]), m++;
    }
    dist[s] = place_shift_distance(score, m);
    if (dist[s] < dist[best]) best = s;
  }
  return best;
}

}  // extern "C"

#ifdef HOSTCHECK_PLACE_MAIN
#include <math.h>
int main() {
  uint64_t state = 88172645463325252ull;
  auto rnd = [&]() {
    state ^= state << 13, state ^= state >> 7, state ^= state << 17;
    return (double)(state >> 11) / 9007199254740992.0;
  };
  const uint32_t shapes[4][2] = {{1, 3}, {3, 5}, {20, 60}, {64, 360}};
  uint64_t total = 0, placed = 0;
  for (int sh = 0; sh < 4; sh++) {
    const uint32_t R = shapes[sh][0], S = shapes[sh][1];
    const double L = 80.0;
    std::vector<double> dirs(2 * (size_t)S);
    hostcheck_place_dirs(S, dirs.data());
    std::vector<double> pts;
    for (int i = 0; i < 4000; i++) pts.insert(pts.end(), {rnd() * 200.0 - 100.0, rnd() * 200.0 - 100.0, rnd() * 16.0 - 4.0});
    for (uint32_t k = 0; k < S; k++)  // on the sector boundaries, scaled by powers of two
      for (double rho : {0.25, 8.0}) pts.insert(pts.end(), {rho * dirs[2 * k], rho * dirs[2 * k + 1], rnd() - 0.5});
    for (uint32_t r = 0; r <= R; r++) {  // on the ring boundaries and one ulp either side
      const double b = L * r / R;
      pts.insert(pts.end(), {b, 0.0, 1.0, nextafter(b, 0.0), 0.0, 1.0, nextafter(b, 1e9), 0.0, 1.0});
    }
    pts.insert(pts.end(), {0.0, 0.0, 0.0, 0.0, 0.0, 3.0, NAN, 1.0, 2.0, 1.0, INFINITY, 2.0, 1.0, 2.0, -INFINITY, 1e-51, 0.0, 0.0, 1e-50, 1e-50, 0.0,
                           1e154, 1e154, 1e154, 1e150, -1e150, 1e149, 1e-49, 1e-49, -1e-49, -0.0, 2.0, -0.0, 3.0, 4.0, -2.0, 3.0, 4.0, -2.5,
                           3.0, 4.0, 1021.984375, 3.0, 4.0, 1021.96875, 3.0, 4.0, 1e150, 3.0, 4.0, -1e150});
    const uint64_t n = pts.size() / 3;
    std::vector<uint32_t> cell(n), code(n);
    hostcheck_place_cells(R, S, L, 2.0, 64.0, dirs.data(), pts.data(), n, cell.data(), code.data());
    const OrgTables t{dirs.data(), nullptr, nullptr, 0u, 0u, S, 0u};
    for (uint64_t i = 0; i < n; i++) {
      const double x = pts[3 * i], y = pts[3 * i + 1];
      total++;
      if (cell[i] == kPlaceNoCell) continue;
      if (cell[i] >= R * S) return printf("%u x %u point %llu: cell %u out of range\n", R, S, (unsigned long long)i, cell[i]), 1;
      if (code[i] < 1 || code[i] > 65535) return printf("%u x %u point %llu: code %u\n", R, S, (unsigned long long)i, code[i]), 1;
      uint32_t ncol = 0, c_ref = 0;
      for (uint32_t k = 0; k < S; k++)
        if (organize_side(t, k, x, y) && !organize_side(t, k + 1 == S ? 0 : k + 1, x, y)) ncol++, c_ref = k;
      if (ncol != 1) return printf("%u x %u point %llu has %u sectors\n", R, S, (unsigned long long)i, ncol), 1;
      if (cell[i] % S != c_ref) return printf("%u x %u point %llu: sector %u, plain scan %u\n", R, S, (unsigned long long)i, cell[i] % S, c_ref), 1;
      placed++;
    }
    // a descriptor against its rolled copies, against all 65535 and against nothing
    std::vector<uint16_t> q((size_t)R * S), e((size_t)R * S), full((size_t)R * S, 65535), none((size_t)R * S, 0);
    std::vector<double> dist(S);
    for (size_t i = 0; i < q.size(); i++) q[i] = rnd() < 0.3 ? 0 : (uint16_t)(1 + rnd() * 3000.0);
    for (uint32_t j = 0; j < S; j++) q[j] = (uint16_t)(j + 1);  // (ring 0 differs in every sector: no two shifts alike)
    for (uint32_t s = 0; s < S; s += (S > 60 ? 37 : 1)) {
      for (uint32_t r = 0; r < R; r++)
        for (uint32_t j = 0; j < S; j++) e[r * S + (j + s) % S] = q[r * S + j];
      const uint32_t best = hostcheck_place_pair(q.data(), e.data(), R, S, dist.data());
      // (one ring: every column is one number, every cosine 1 and every shift ties at 0; the lowest wins)
      if (best != (R == 1 ? 0u : s) || dist[s] != 0.0) return printf("%u x %u: rolled by %u found at %u with %g\n", R, S, s, best, dist[s]), 1;
    }
    if (hostcheck_place_pair(full.data(), full.data(), R, S, dist.data()) != 0 || dist[0] != 0.0) return printf("%u x %u: full against full\n", R, S), 1;
    if (hostcheck_place_pair(none.data(), full.data(), R, S, dist.data()) != 0 || dist[0] != 1.0) return printf("%u x %u: none against full\n", R, S), 1;
  }
  if (place_cos_q(10, 1, 1) != kPlaceCosOne || place_cos_q(0, 5, 7) != 0) return printf("cosine clamp\n"), 1;
  if (placed == 0) return printf("no point was placed\n"), 1;
  printf("hostcheck_place ok: %llu points, %llu placed\n", (unsigned long long)total, (unsigned long long)placed);
  return 0;
}
#endif
