// surfel_math.h — the arithmetic of the surfel map (loamx.h, "surfel map"): what a point adds to its voxel (16-bit offsets, their
// products, the view terms) and surfel_finish, the ONE function that turns a voxel's integer sums into its record: the emit
// kernel, the query kernel and tests/hostcheck_surfel all call it. Host + device, like cloudmap_math.h, whose validity, voxel and
// offset it reuses unchanged. Every product, quotient, sum and difference is rounded on its own (-ffp-contract=off), in the order
// written; sqrt is the only libm call (inside jacobi_rotate of reg_math.h, the registration's own Jacobi).
#pragma once
#include "../../include/loamx.h"
#include "cloudmap_math.h"

namespace loamx {

constexpr double kSurfelUnit = 65536.0;             // offsets inside a voxel count in steps of leaf / 2^16
constexpr double kSurfelViewUnit = 256.0;           // view terms count in steps of leaf / 256
constexpr double kSurfelViewClamp = 1073741824.0;   // ... and are clamped to [-2^30, 2^30]: 2^32 - 2 of them stay below 2^62
constexpr double kSurfelTwo64 = 18446744073709551616.0;
// the thirteen values of a point, and of a slot: s[3], S[6] (xx xy xz yy yz zz), W[3] as 64-bit words, then the count
constexpr int kSurfelMoments = 12;

// q[a] = u[a] >> 16 of the cloud map's 32-bit offset: a product q q < 2^32, so 2^32 - 2 of them cannot wrap 64 bits
LOAMX_HD uint32_t surfel_offset(uint32_t u) { return u >> 16; }

// w = floor(clamp(((o - p') / leaf) 256)): the direction back to the sensor in steps of leaf / 256. The clamp is written so that
// a NaN (which no used point produces) becomes the lower bound instead of an undefined conversion.
LOAMX_HD int64_t surfel_view(double o, double p, double leaf) {
  const double d = o - p;
  const double t = d / leaf;
  double x = t * kSurfelViewUnit;
  if (!(x >= -kSurfelViewClamp)) x = -kSurfelViewClamp;
  if (x > kSurfelViewClamp) x = kSurfelViewClamp;
  return (int64_t)floor(x);
}

// the twelve 64-bit words a used point adds (the view terms in two's complement): m[0..2] = q, m[3..8] = q q, m[9..11] = w
LOAMX_HD void surfel_point(const uint32_t u[3], Vec3 o, Vec3 p, double leaf, unsigned long long m[kSurfelMoments]) {
  const unsigned long long q0 = surfel_offset(u[0]), q1 = surfel_offset(u[1]), q2 = surfel_offset(u[2]);
  m[0] = q0, m[1] = q1, m[2] = q2;
  m[3] = q0 * q0, m[4] = q0 * q1, m[5] = q0 * q2, m[6] = q1 * q1, m[7] = q1 * q2, m[8] = q2 * q2;
  m[9] = (unsigned long long)surfel_view(o.x, p.x, leaf);
  m[10] = (unsigned long long)surfel_view(o.y, p.y, leaf);
  m[11] = (unsigned long long)surfel_view(o.z, p.z, leaf);
}

// N = count S - sa sb, exact in 128 bits (each term is below 2^96), to FP64 as sign ((double) hi 2^64 + (double) lo) of the
// magnitude's halves. (A 128-bit value is never cast to double itself: the device has no helper for that.)
LOAMX_HD double surfel_numerator(uint32_t count, uint64_t S, uint64_t sa, uint64_t sb) {
  const unsigned __int128 A = (unsigned __int128)count * S, B = (unsigned __int128)sa * sb;
  const bool neg = A < B;
  const unsigned __int128 mag = neg ? B - A : A - B;
  const uint64_t hi = (uint64_t)(mag >> 64), lo = (uint64_t)mag;
  const double d = (double)hi * kSurfelTwo64 + (double)lo;
  return neg ? -d : d;
}

// The record of a voxel. s, S: the sums of the offsets and of their products; W: the view sums; count >= 1.
LOAMX_HD loamx_surfel surfel_finish(uint64_t key, const uint64_t s[3], const uint64_t S[6], const int64_t W[3], uint32_t count, uint32_t first,
                                    double leaf) {
  loamx_surfel r;
  const double dn = (double)count, h = leaf / kSurfelUnit;
  for (int a = 0; a < 3; a++) r.mean[a] = ((double)cloud_key_coord(key, a) + ((double)s[a] / dn) / kSurfelUnit) * leaf;
  const double dn2 = dn * dn, h2 = h * h;
  r.cov[0] = (surfel_numerator(count, S[0], s[0], s[0]) / dn2) * h2;
  r.cov[1] = (surfel_numerator(count, S[1], s[0], s[1]) / dn2) * h2;
  r.cov[2] = (surfel_numerator(count, S[2], s[0], s[2]) / dn2) * h2;
  r.cov[3] = (surfel_numerator(count, S[3], s[1], s[1]) / dn2) * h2;
  r.cov[4] = (surfel_numerator(count, S[4], s[1], s[2]) / dn2) * h2;
  r.cov[5] = (surfel_numerator(count, S[5], s[2], s[2]) / dn2) * h2;
  // cyclic Jacobi as fit_line (reg_math.h) runs it; columns of V are eigenvectors
  double a00 = r.cov[0], a01 = r.cov[1], a02 = r.cov[2], a11 = r.cov[3], a12 = r.cov[4], a22 = r.cov[5];
  double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;
  for (int sweep = 0; sweep < 32; sweep++) {
    if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
    jacobi_rotate(a00, a11, a01, a02, a12, v00, v10, v20, v01, v11, v21);  // (p,q,r) = (0,1,2)
    jacobi_rotate(a00, a22, a02, a01, a12, v00, v10, v20, v02, v12, v22);  // (0,2,1)
    jacobi_rotate(a11, a22, a12, a01, a02, v01, v11, v21, v02, v12, v22);  // (1,2,0)
  }
  // ascending, stable (an insertion sort of three: ties keep column order), not clamped at 0
  double e0 = a00, e1 = a11, e2 = a22;
  int c0 = 0, c1 = 1, c2 = 2;
  if (e1 < e0) { double t = e0; e0 = e1; e1 = t; int ti = c0; c0 = c1; c1 = ti; }
  if (e2 < e1) {
    { double t = e1; e1 = e2; e2 = t; int ti = c1; c1 = c2; c2 = ti; }
    if (e1 < e0) { double t = e0; e0 = e1; e1 = t; int ti = c0; c0 = c1; c1 = ti; }
  }
  (void)c1, (void)c2;
  r.eval[0] = e0, r.eval[1] = e1, r.eval[2] = e2;
  double n0 = c0 == 0 ? v00 : (c0 == 1 ? v01 : v02);
  double n1 = c0 == 0 ? v10 : (c0 == 1 ? v11 : v12);
  double n2 = c0 == 0 ? v20 : (c0 == 1 ? v21 : v22);
  // towards where the voxel was seen from
  const double dot = n0 * (double)W[0] + n1 * (double)W[1] + n2 * (double)W[2];
  bool flip = dot < 0.0;
  if (dot == 0.0) {  // the component of largest magnitude decides, the lowest axis on ties
    double big = n0;
    if (fabs(n1) > fabs(big)) big = n1;
    if (fabs(n2) > fabs(big)) big = n2;
    flip = big < 0.0;
  }
  if (flip) n0 = -n0, n1 = -n1, n2 = -n2;
  r.normal[0] = n0, r.normal[1] = n1, r.normal[2] = n2;
  r.count = count, r.first = first;
  return r;
}

// the signed distance of p to the surfel's plane: normal . (p - mean), left to right
LOAMX_HD double surfel_distance(const loamx_surfel& r, Vec3 p) {
  return r.normal[0] * (p.x - r.mean[0]) + r.normal[1] * (p.y - r.mean[1]) + r.normal[2] * (p.z - r.mean[2]);
}

}  // namespace loamx
