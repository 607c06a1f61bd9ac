// info_math.h — the registration information matrix (loamx.h: loamx_reg_information): one residual row in the user-facing
// tangent basis, its accumulation into the normal equations, and the eigen-decomposition of the 6x6 result.
//
// Basis. For a pose T = target_T_source the perturbation is applied on the LEFT, T <- Exp([omega, t]) o T: omega is a rotation
// vector in radians about the axes of the TARGET frame, t a translation in metres along them, rotation first. A moved point
// v = T.act(p) then becomes v + omega x v + t to first order, so a residual r(v) with gradient g = dr/dv has the row
//     J = [ v x g , g ]                       (g . (omega x v) = omega . (v x g)).
// (The solver's own rows — residual_accumulate in reg_math.h — live in Ceres' half-angle QuaternionManifold basis on
// Eigen-ordered storage; nothing outside the solver sees that basis.)
// Shared by host and device code like map_math.h / deskew_math.h: tests/hostcheck_info compiles this file with g++.
#pragma once
#include "reg_math.h"

namespace loamx {

struct InfoRow {
  double J[6];  // [v x g, g]
  double r;     // residual (>= 0)
};

// The row of one association record: v = the moved point; plane: prim = normal(3), d; edge: prim = a(3), b(3).
//   plane  s = n.v - d, r = |s|, g = copysign(1, s) n
//   edge   c = (v - a) x (v - b), r = |c| / |a - b|, g = ((a - b) x c) / (|c| |a - b|)
// false: some entry is not finite (an edge point exactly on its line has |c| = 0; a line with a = b has no direction).
LOAMX_HD bool info_row(bool is_plane, Vec3 v, const double prim[6], InfoRow& row) {
  Vec3 g;
  double r;
  if (is_plane) {
    const Vec3 n = v3(prim[0], prim[1], prim[2]);
    const double s = vdot(n, v) - prim[3];
    r = fabs(s);
    g = vscale(copysign(1.0, s), n);
  } else {
    const Vec3 a = v3(prim[0], prim[1], prim[2]), b = v3(prim[3], prim[4], prim[5]);
    const Vec3 c = vcross(vsub(v, a), vsub(v, b));
    const double cn = vnorm(c);
    const Vec3 ab = vsub(a, b);
    const double den = vnorm(ab);
    r = cn / den;
    g = vscale(1.0 / (cn * den), vcross(ab, c));
  }
  const Vec3 vxg = vcross(v, g);
  row.J[0] = vxg.x, row.J[1] = vxg.y, row.J[2] = vxg.z, row.J[3] = g.x, row.J[4] = g.y, row.J[5] = g.z;
  row.r = r;
  bool finite = (r - r == 0.0);
#pragma unroll
  for (int j = 0; j < 6; j++) finite = finite && (row.J[j] - row.J[j] == 0.0);
  return finite;
}

// HuberLoss(1.0) as the solver applies it (residual_accumulate): for r^2 > 1 row and residual are scaled by sqrt(1 / r).
// true: the row was in that region.
LOAMX_HD bool info_huber(InfoRow& row) {
  const double s2 = row.r * row.r;
  if (!(s2 > 1.0)) return false;
  double rho1 = 1.0 / sqrt(s2);
  if (rho1 < kDblMin) rho1 = kDblMin;
  const double sc = sqrt(rho1);
#pragma unroll
  for (int j = 0; j < 6; j++) row.J[j] *= sc;
  row.r *= sc;
  return true;
}

// sums[0..20] upper triangle of J^T J (row-major: 00 01 .. 05 11 12 ..), [21..26] J^T r, [27] r^2 — of the scaled rows
constexpr int kInfoSums = 28;
struct InfoAcc {
  double s[kInfoSums];
  uint32_t n_edge, n_plane, n_huber, n_dropped;
};
LOAMX_HD void info_acc_clear(InfoAcc& A) {
#pragma unroll
  for (int j = 0; j < kInfoSums; j++) A.s[j] = 0.0;
  A.n_edge = A.n_plane = A.n_huber = A.n_dropped = 0u;
}
// one VALID association record into the sums (a non-finite row is counted in n_dropped and adds nothing)
LOAMX_HD void info_accumulate(bool is_plane, Vec3 v, const double prim[6], InfoAcc& A) {
  InfoRow row;
  if (!info_row(is_plane, v, prim, row)) {
    A.n_dropped++;
    return;
  }
  if (info_huber(row)) A.n_huber++;
  if (is_plane) A.n_plane++;
  else A.n_edge++;
  int t = 0;
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int j = i; j < 6; j++) A.s[t++] += row.J[i] * row.J[j];
#pragma unroll
  for (int j = 0; j < 6; j++) A.s[21 + j] += row.J[j] * row.r;
  A.s[27] += row.r * row.r;
}

// upper triangle (row-major, 21 entries) -> full row-major 6x6 whose two halves hold the same bits
LOAMX_HD void info_mirror(const double tri[21], double H[36]) {
  int t = 0;
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int j = i; j < 6; j++, t++) H[6 * i + j] = H[6 * j + i] = tri[t];
}

/* Eigen-decomposition of a symmetric 6x6 matrix (only the upper triangle of H is read): cyclic Jacobi in FP64.
 *   schedule   every sweep visits the 15 pairs (p, q) in row order (0,1) (0,2) .. (4,5); each visit is a function instantiated for
 *              its pair, so every index is a compile-time constant and a device build keeps both matrices in registers
 *   rotation   skipped when |a_pq| <= 2^-53 sqrt(|a_pp| |a_qq|) (or a_pq == 0): the entry can no longer move either eigenvalue
 *              by a unit in its last place. Rutishauser's formulas: t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)) with
 *              theta = (a_qq - a_pp) / (2 a_pq), c = 1 / sqrt(t^2 + 1), s = t c, tau = s / (1 + c)
 *   sweep cap  kInfoEigSweeps; a sweep that rotates nothing ends the iteration (6 - 10 sweeps in practice)
 *   order      eigenvalues ascending (a stable exchange sort: equal eigenvalues keep the order of their columns, so the zero
 *              matrix returns the identity)
 *   sign       row i of `evec` is the unit eigenvector of eval[i]; its largest-magnitude component (the one of lowest index when
 *              several tie) is positive
 * Returns the number of sweeps that rotated something. */
constexpr int kInfoEigSweeps = 30;

template <int P, int Q>
LOAMX_HD bool info_jacobi_rotate(double (&a)[6][6], double (&v)[6][6]) {
  const double apq = a[P][Q], app = a[P][P], aqq = a[Q][Q];
  if (apq == 0.0 || fabs(apq) <= 1.1102230246251565e-16 * (sqrt(fabs(app)) * sqrt(fabs(aqq)))) return false;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
  a[P][P] = app - t * apq;
  a[Q][Q] = aqq + t * apq;
  a[P][Q] = 0.0;
#pragma unroll
  for (int k = 0; k < 6; k++) {
    if (k != P && k != Q) {  // (entry (k, P) of the symmetric matrix lives in the upper triangle)
      double& akp = k < P ? a[k][P] : a[P][k];
      double& akq = k < Q ? a[k][Q] : a[Q][k];
      const double x = akp, y = akq;
      akp = x - s * (y + tau * x);
      akq = y + s * (x - tau * y);
    }
    const double x = v[k][P], y = v[k][Q];
    v[k][P] = x - s * (y + tau * x);
    v[k][Q] = y + s * (x - tau * y);
  }
  return true;
}

LOAMX_HD int info_eig6(const double H[36], double eval[6], double evec[36]) {
  double a[6][6], v[6][6];
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int j = 0; j < 6; j++) a[i][j] = j >= i ? H[6 * i + j] : 0.0, v[i][j] = i == j ? 1.0 : 0.0;
  int sweeps = 0;
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll 1
#endif
  for (int sweep = 0; sweep < kInfoEigSweeps; sweep++) {
    bool any = false;
    any |= info_jacobi_rotate<0, 1>(a, v), any |= info_jacobi_rotate<0, 2>(a, v), any |= info_jacobi_rotate<0, 3>(a, v);
    any |= info_jacobi_rotate<0, 4>(a, v), any |= info_jacobi_rotate<0, 5>(a, v), any |= info_jacobi_rotate<1, 2>(a, v);
    any |= info_jacobi_rotate<1, 3>(a, v), any |= info_jacobi_rotate<1, 4>(a, v), any |= info_jacobi_rotate<1, 5>(a, v);
    any |= info_jacobi_rotate<2, 3>(a, v), any |= info_jacobi_rotate<2, 4>(a, v), any |= info_jacobi_rotate<2, 5>(a, v);
    any |= info_jacobi_rotate<3, 4>(a, v), any |= info_jacobi_rotate<3, 5>(a, v), any |= info_jacobi_rotate<4, 5>(a, v);
    if (!any) break;
    sweeps++;
  }
  double d[6];
#pragma unroll
  for (int i = 0; i < 6; i++) d[i] = a[i][i];
#pragma unroll
  for (int pass = 0; pass < 5; pass++)
#pragma unroll
    for (int i = 0; i + 1 < 6 - pass; i++)
      if (d[i] > d[i + 1]) {
        const double td = d[i];
        d[i] = d[i + 1], d[i + 1] = td;
#pragma unroll
        for (int k = 0; k < 6; k++) {
          const double tv = v[k][i];
          v[k][i] = v[k][i + 1], v[k][i + 1] = tv;
        }
      }
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double big = v[0][i];
#pragma unroll
    for (int k = 1; k < 6; k++)
      if (fabs(v[k][i]) > fabs(big)) big = v[k][i];
    const double sg = big < 0.0 ? -1.0 : 1.0;
    eval[i] = d[i];
#pragma unroll
    for (int k = 0; k < 6; k++) evec[6 * i + k] = sg * v[k][i];
  }
  return sweeps;
}

}  // namespace loamx
