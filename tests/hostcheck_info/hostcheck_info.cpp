// TEST-ONLY: info_math.h (the row, the accumulation and the 6x6 eigen-solve of the registration information matrix) compiled
// for the host behind extern "C" wrappers, for tests/test_info_hostcheck.py and the models of the GPU tests. With
// -DHOSTCHECK_INFO_MAIN the file is a stand-alone program that runs the same wrappers over generated inputs (the `san`
// target builds it with -fsanitize=address,undefined).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../loam_amd/csrc/info_math.h"

using namespace loamx;

extern "C" {

// Row i of record i: kind[i] (0 edge, 1 plane), v[i] (3), prim[i] (6: a, b | n, d, -, -). J_out (n x 6), r_out (n);
// flags_out[i]: bit 0 = the row is finite (it enters the sums), bit 1 = it was in the Huber region. scaled = 0: the row as
// info_row returns it; 1: after info_huber.
void hostcheck_info_rows(uint64_t n, const uint8_t* kind, const double* v, const double* prim, int scaled, double* J_out, double* r_out,
                         uint8_t* flags_out) {
  for (uint64_t i = 0; i < n; i++) {
    InfoRow row;
    const bool ok = info_row(kind[i] != 0, v3(v[3 * i], v[3 * i + 1], v[3 * i + 2]), prim + 6 * i, row);
    bool huber = false;
    if (ok && scaled) huber = info_huber(row);
    for (int j = 0; j < 6; j++) J_out[6 * i + j] = row.J[j];
    r_out[i] = row.r;
    flags_out[i] = (uint8_t)((ok ? 1 : 0) | (huber ? 2 : 0));
  }
}

// the records in order through info_accumulate: sums[28], counters[4] = n_edge, n_plane, n_huber, n_dropped
void hostcheck_info_accumulate(uint64_t n, const uint8_t* kind, const double* v, const double* prim, double* sums, uint32_t* counters) {
  InfoAcc A;
  info_acc_clear(A);
  for (uint64_t i = 0; i < n; i++) info_accumulate(kind[i] != 0, v3(v[3 * i], v[3 * i + 1], v[3 * i + 2]), prim + 6 * i, A);
  for (int j = 0; j < kInfoSums; j++) sums[j] = A.s[j];
  counters[0] = A.n_edge, counters[1] = A.n_plane, counters[2] = A.n_huber, counters[3] = A.n_dropped;
}

void hostcheck_info_mirror(const double* tri, double* H) { info_mirror(tri, H); }

// returns the number of sweeps that rotated something
int hostcheck_info_eig6(const double* H, double* eval, double* evec) { return info_eig6(H, eval, evec); }

int hostcheck_info_sweep_cap() { return kInfoEigSweeps; }

}  // extern "C"

#ifdef HOSTCHECK_INFO_MAIN
#include <math.h>
int main() {
  uint64_t state = 88172645463325252ull;
  auto rnd = [&]() {
    state ^= state << 13, state ^= state >> 7, state ^= state << 17;
    return (double)(state >> 11) / 9007199254740992.0;
  };
  // random records of both kinds, then the special ones: a point on its line, a line without direction, non-finite fields
  std::vector<uint8_t> kind;
  std::vector<double> v, prim;
  auto add = [&](int k, std::initializer_list<double> vv, std::initializer_list<double> pp) {
    kind.push_back((uint8_t)k), v.insert(v.end(), vv), prim.insert(prim.end(), pp);
  };
  for (int i = 0; i < 20000; i++) {
    const double x = rnd() * 240 - 120, y = rnd() * 240 - 120, z = rnd() * 20 - 10;
    if (i & 1) {
      double n[3] = {rnd() - 0.5, rnd() - 0.5, rnd() - 0.5};
      const double nn = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
      add(1, {x, y, z}, {n[0] / nn, n[1] / nn, n[2] / nn, rnd() * 10 - 5, 0.0, 0.0});
    } else {
      add(0, {x, y, z}, {x + rnd(), y + rnd(), z + rnd(), x + rnd() + 0.2, y - rnd(), z + rnd()});
    }
  }
  add(0, {1, 2, 3}, {0, 2, 3, 2, 2, 3});        // on the line: |c| = 0
  add(0, {1, 2, 3}, {4, 4, 4, 4, 4, 4});        // a = b
  add(0, {NAN, 2, 3}, {0, 0, 0, 1, 0, 0});
  add(1, {1, 2, 3}, {0, 0, INFINITY, 1, 0, 0});
  add(1, {0, 0, 3}, {0, 0, 1, 0, 0, 0});        // Huber region
  add(1, {0, 0, 1}, {0, 0, 1, 0, 0, 0});        // exactly r^2 = 1
  const uint64_t n = kind.size();
  std::vector<double> J(6 * n), r(n);
  std::vector<uint8_t> flags(n);
  hostcheck_info_rows(n, kind.data(), v.data(), prim.data(), 1, J.data(), r.data(), flags.data());
  double sums[kInfoSums], H[36], eval[6], evec[36];
  uint32_t c[4];
  hostcheck_info_accumulate(n, kind.data(), v.data(), prim.data(), sums, c);
  if (c[3] != 4 || c[0] + c[1] + c[3] != n || c[2] == 0) {
    printf("unexpected counters %u %u %u %u of %llu\n", c[0], c[1], c[2], c[3], (unsigned long long)n);
    return 1;
  }
  hostcheck_info_mirror(sums, H);
  const int sweeps = hostcheck_info_eig6(H, eval, evec);
  for (int i = 0; i + 1 < 6; i++)
    if (!(eval[i] <= eval[i + 1])) return 1;
  // the matrices a record can hold at its edges: zero, diagonal, a rank-one matrix, huge and tiny scales
  double Z[36] = {0};
  if (hostcheck_info_eig6(Z, eval, evec) != 0 || evec[0] != 1.0 || evec[35] != 1.0) return 1;
  for (double scale : {1e-300, 1.0, 1e150}) {
    double M[36];
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) M[6 * i + j] = scale * (double)((i + 1) * (j + 1));
    if (hostcheck_info_eig6(M, eval, evec) > hostcheck_info_sweep_cap()) return 1;
  }
  printf("hostcheck_info ok: %llu records, %u + %u rows, %u huber, %u dropped, %d sweeps\n", (unsigned long long)n, c[0], c[1], c[2], c[3], sweeps);
  return 0;
}
#endif
