// TEST-ONLY: deskew_math.h (the per-column and per-point arithmetic of deskew_kernel) compiled for the host behind
// extern "C" wrappers, for tests/test_deskew_hostcheck.py. With -DHOSTCHECK_DESKEW_MAIN the file is a stand-alone program
// that runs the same wrappers over generated inputs (the `san` target builds it with -fsanitize=address,undefined).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../loam_amd/csrc/deskew_math.h"

using namespace loamx;

extern "C" {

// what deskew_kernel computes once per thread: motion[i] (7 doubles as in memory), tau[i], rho[i] -> q[i] (the 4 numbers
// deskew_load_motion hands on) and col[i] = m (9, row-major) | d (3)
void hostcheck_deskew_columns(const double* motion, const double* tau, const double* rho, uint64_t n, double* q_out, double* col) {
  for (uint64_t i = 0; i < n; i++) {
    double q[4], t[3];
    deskew_load_motion(motion + 7 * i, q, t);
    const DeskewColumn c = deskew_column(q, t, tau[i], rho[i]);
    for (int k = 0; k < 4; k++) q_out[4 * i + k] = q[k];
    for (int k = 0; k < 9; k++) col[12 * i + k] = c.m[k];
    for (int k = 0; k < 3; k++) col[12 * i + 9 + k] = c.d[k];
  }
}

// deskew_point of pts[i] (n x 3) under ONE column (12 doubles as above); moved[i] = 0: the point is to be copied (out[i] is
// then the input, as the kernel stores it)
void hostcheck_deskew_points(const double* col, const double* pts, uint64_t n, double* out, uint8_t* moved) {
  DeskewColumn c;
  for (int k = 0; k < 9; k++) c.m[k] = col[k];
  for (int k = 0; k < 3; k++) c.d[k] = col[9 + k];
  for (uint64_t i = 0; i < n; i++) {
    double r[3];
    moved[i] = deskew_point(c, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], r) ? 1 : 0;
    for (int k = 0; k < 3; k++) out[3 * i + k] = moved[i] ? r[k] : pts[3 * i + k];
  }
}

}  // extern "C"

#ifdef HOSTCHECK_DESKEW_MAIN
#include <math.h>
int main() {
  // random motions with angles from 1e-15 to pi, scaled and negated quaternions, the small-angle seam, half turns about
  // w = +-0, the zero quaternion; every tau, rho of a coarse grid; points with zeros and non-finite values
  uint64_t state = 88172645463325252ull;
  auto rnd = [&]() {
    state ^= state << 13, state ^= state >> 7, state ^= state << 17;
    return (double)(state >> 11) / 9007199254740992.0;
  };
  std::vector<double> motion, tau, rho;
  const double frac[5] = {0.0, 1.0 / 1024.0, 0.5, 1.0 - 1.0 / 1024.0, 1.0};
  auto add = [&](double x, double y, double z, double w, double scale) {
    for (int a = 0; a < 5; a++)
      for (int b = 0; b < 5; b++) {
        motion.insert(motion.end(), {x * scale, y * scale, z * scale, w * scale, rnd() * 10.0 - 5.0, rnd() * 10.0 - 5.0, rnd() * 10.0 - 5.0});
        tau.push_back(frac[a]), rho.push_back(frac[b]);
      }
  };
  const double scales[6] = {1.0, 1e-3, -3.0, 1e3, 1e-150, 1e150};
  for (int i = 0; i < 400; i++) {
    const double angle = exp(log(1e-15) + rnd() * (log(M_PI) - log(1e-15)));
    double ax = rnd() - 0.5, ay = rnd() - 0.5, az = rnd() - 0.5;
    const double an = sqrt(ax * ax + ay * ay + az * az) + 1e-300, s = sin(angle / 2) / an;
    add(ax * s, ay * s, az * s, cos(angle / 2), scales[i % 6]);
  }
  for (double vn : {0.0, 1e-14, 9.99e-13, 1e-12, 1.01e-12, 1e-10}) add(vn, 0.0, 0.0, 1.0, 1.0), add(0.0, -0.6 * vn, 0.8 * vn, 1.0, -3.0);
  for (double w : {0.0, -0.0, 1e-300, -1e-300, 1e-9, -1e-9}) add(0.6, 0.0, -0.8, w, 1.0);
  add(0.0, 0.0, 0.0, 1.0, 1.0), add(0.0, 0.0, 0.0, 1.0, -2.5), add(0.0, 0.0, 0.0, 0.0, 1.0), add(0.3, 0.1, 0.2, 0.9, 1e-170);
  const uint64_t n = tau.size();
  std::vector<double> q(4 * n), col(12 * n);
  hostcheck_deskew_columns(motion.data(), tau.data(), rho.data(), n, q.data(), col.data());
  std::vector<double> pts;
  for (int i = 0; i < 1000; i++) pts.insert(pts.end(), {rnd() * 200.0 - 100.0, rnd() * 200.0 - 100.0, rnd() * 200.0 - 100.0});
  pts.insert(pts.end(), {0.0, 0.0, 0.0, NAN, 1.0, 2.0, 3.0, -INFINITY, 2.0, -0.0, 0.0, -0.0, 1e308, -1e308, 1e308});
  const uint64_t np = pts.size() / 3;
  std::vector<double> out(3 * np);
  std::vector<uint8_t> moved(np);
  uint64_t n_moved = 0, n_nan_cols = 0;
  for (uint64_t i = 0; i < n; i++) {
    hostcheck_deskew_points(col.data() + 12 * i, pts.data(), np, out.data(), moved.data());
    for (uint64_t k = 0; k < np; k++) n_moved += moved[k];
    n_nan_cols += col[12 * i] != col[12 * i] ? 1 : 0;
  }
  if (n_moved != n * (np - 4)) {  // the two zero points, the NaN and the -Inf point are copied; 1e308 is finite and moves
    printf("moved %llu points, expected %llu\n", (unsigned long long)n_moved, (unsigned long long)(n * (np - 4)));
    return 1;
  }
  if (n_nan_cols != 50) {  // the zero quaternion and the one whose squares underflow, 25 (tau, rho) each
    printf("%llu columns are NaN, expected 50\n", (unsigned long long)n_nan_cols);
    return 1;
  }
  printf("hostcheck_deskew ok: %llu columns, %llu points each\n", (unsigned long long)n, (unsigned long long)np);
  return 0;
}
#endif
