// deskew_math.h — per-point motion correction of a scan (loamx.h: loamx_deskew_scans_dev). The reference leaves
// "steps to dewarp pointclouds" to its users (README, Example Usage); this is that step for a sweep whose motion is known.
//
// Convention. A scan is row-major [line][column]; column c was measured at sweep fraction tau = c / points_per_line.
// motion = (q, t) is start_T_end of the sweep: the pose of the sensor at the end of the sweep in its frame at the start.
// The sensor's pose at fraction tau is T(tau) = (slerp(identity, q, tau), tau * t) — constant velocity, q taken along the
// short arc. A point p measured at tau is moved into the sensor frame at fraction rho:
//     p_out = R(rho)^T (R(tau) p + (tau - rho) t)
// rho = 1 is the frame at the end of the sweep (LOAM's convention), rho = 0 the frame at its start.
// The rotations are applied as the rotation matrices of unit quaternions (Pose3d::matrix's formula), so an identity
// motion gives the identity matrix and a zero offset exactly and the finite, non-zero input comes back bit for bit (a
// coordinate that is -0.0 next to non-zero ones may come back as +0.0).
// Shared by host and device code like extract_math.h / reg_math.h.
#pragma once
#include "reg_math.h"

namespace loamx {

// what one column of one scan does to its points: p_out = m p + d (m row-major)
struct DeskewColumn {
  double m[9];
  double d[3];
};

// the motion as read from memory: unit quaternion with w >= 0 (short arc), translation
LOAMX_HD void deskew_load_motion(const double* __restrict__ mo, double q[4], double t[3]) {
  const double n = sqrt(mo[0] * mo[0] + mo[1] * mo[1] + mo[2] * mo[2] + mo[3] * mo[3]);
  const double sn = mo[3] < 0.0 ? -n : n;
  for (int i = 0; i < 4; i++) q[i] = mo[i] / sn;  // (a division: a unit or axis-aligned quaternion comes through exactly)
  for (int i = 0; i < 3; i++) t[i] = mo[4 + i];
}

// slerp(identity, q, tau) for a unit q with w >= 0: theta = 2 atan2(|v|, w), result (sin(tau theta / 2) v / |v|, cos(tau theta / 2));
// below |v| = 1e-12 the angle is its sine: (tau v, 1), normalised
LOAMX_HD void deskew_slerp(const double q[4], double tau, double out[4]) {
  const double vn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
  if (vn < 1e-12) {
    const double x = tau * q[0], y = tau * q[1], z = tau * q[2];
    const double inv = 1.0 / sqrt(x * x + y * y + z * z + 1.0);
    out[0] = x * inv, out[1] = y * inv, out[2] = z * inv, out[3] = inv;
    return;
  }
  const double half = tau * atan2(vn, q[3]);
  const double s = sin(half) / vn;
  out[0] = s * q[0], out[1] = s * q[1], out[2] = s * q[2], out[3] = cos(half);
}

// rotation matrix of a unit quaternion, row-major (include/loam/geometry.h: Pose3d::matrix)
LOAMX_HD void deskew_rotation(const double q[4], double r[9]) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  r[0] = 1 - (tyy + tzz), r[1] = txy - twz, r[2] = txz + twy;
  r[3] = txy + twz, r[4] = 1 - (txx + tzz), r[5] = tyz - twx;
  r[6] = txz - twy, r[7] = tyz + twx, r[8] = 1 - (txx + tyy);
}

// m = R(rho)^T R(tau), d = R(rho)^T ((tau - rho) t)
LOAMX_HD DeskewColumn deskew_column(const double q[4], const double t[3], double tau, double rho) {
  double qt[4], qr[4], rt[9], rr[9];
  deskew_slerp(q, tau, qt);
  deskew_slerp(q, rho, qr);
  deskew_rotation(qt, rt);
  deskew_rotation(qr, rr);
  DeskewColumn c;
  const double dt = tau - rho;
  const double u[3] = {dt * t[0], dt * t[1], dt * t[2]};
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) c.m[3 * i + j] = rr[i] * rt[j] + rr[3 + i] * rt[3 + j] + rr[6 + i] * rt[6 + j];
    c.d[i] = rr[i] * u[0] + rr[3 + i] * u[1] + rr[6 + i] * u[2];
  }
  return c;
}

// one point; all three coordinates exactly zero (the no-return beam) or any of them not finite: left as it is (false)
LOAMX_HD bool deskew_point(const DeskewColumn& c, double x, double y, double z, double out[3]) {
  const bool zero = x == 0.0 && y == 0.0 && z == 0.0;
  const bool finite = fabs(x) <= 1.7976931348623157e308 && fabs(y) <= 1.7976931348623157e308 && fabs(z) <= 1.7976931348623157e308;
  if (zero || !finite) return false;
  out[0] = c.m[0] * x + c.m[1] * y + c.m[2] * z + c.d[0];
  out[1] = c.m[3] * x + c.m[4] * y + c.m[5] * z + c.d[1];
  out[2] = c.m[6] * x + c.m[7] * y + c.m[8] * z + c.d[2];
  return true;
}

}  // namespace loamx
