// Keyframe-to-current pose (rebvio_hip_map_keyframe_pose; include/rebvio_hip.h is the definition): the term of one correspondence
// and the O(1) math of one Gauss-Newton step - fixed-order sum of the workgroup partials, 6x6 Cholesky solve, SE3 update. One
// source for the device (k_kf_pose_sums / k_kf_pose_step, track.hip) and the host (rebvio_hip_test_kf_pose_host, api.hip), as
// glue.hpp / hostmath.hpp do it. fp64 throughout; every + - * / and sqrt is an operation of its own (-ffp-contract=off).
#pragma once

#include "hostmath.hpp"  // RH_HD
#include "rebvio_hip.h"

namespace rh {
namespace kfp {

constexpr int kSums = 28;  // 21 unique w J_a J_b (a <= b, row-major), 6 w J_a e, the cost

// index of H(a, b), a <= b, among the 21
RH_HD inline int h_index(int a, int b) { return a * 6 - a * (a - 1) / 2 + (b - a); }

// the test of cloud_pass (track.hip) on the keyframe side of a correspondence
RH_HD inline bool filter_pass(const rebvio_hip_cloud_filter& f, float rho, float sigma_rho, unsigned matches) {
  return matches >= f.min_matches && rho >= f.rho_min && rho <= f.rho_max && sigma_rho <= f.max_rel_sigma * rho;
}

// One term: the keyframe keyline (kx, ky, rho: pos_img and rho of the snapshot) seen as the current keyline (qx, qy: pos_img; gx, gy:
// gradient) under the pose (R, t). false: skipped (positive tests, a NaN skips), v untouched. true: v = the term's 28 addends.
RH_HD inline bool term(float fm, float kx, float ky, float rho_f, float qx_f, float qy_f, float gx_f, float gy_f, const double* R,
                       const double* t, double huber, double* v) {
  const double a = (double)(kx / fm), b = (double)(ky / fm), rho = (double)rho_f;
  const double qx = (double)(qx_f / fm), qy = (double)(qy_f / fm);
  const double gx = (double)gx_f, gy = (double)gy_f;
  const double g2 = gx * gx + gy * gy;
  if (!(g2 > 0.0 && g2 < HUGE_VAL)) return false;
  const double gn = sqrt(g2);
  const double nx = gx / gn, ny = gy / gn;
  const double Zx = (R[0] * a + R[1] * b) + R[2];
  const double Zy = (R[3] * a + R[4] * b) + R[5];
  const double Zz = (R[6] * a + R[7] * b) + R[8];
  const double Yx = Zx + rho * t[0], Yy = Zy + rho * t[1], Yz = Zz + rho * t[2];
  if (!(Yz > 0.0)) return false;
  const double px = Yx / Yz, py = Yy / Yz;
  const double f = (double)fm;
  const double e = f * (nx * (px - qx) + ny * (py - qy));
  const double cx = (f * nx) / Yz, cy = (f * ny) / Yz;
  const double cz = -(cx * px + cy * py);
  double J[6];
  J[0] = rho * cx;
  J[1] = rho * cy;
  J[2] = rho * cz;
  J[3] = Zy * cz - Zz * cy;
  J[4] = Zz * cx - Zx * cz;
  J[5] = Zx * cy - Zy * cx;
  const double ae = fabs(e);
  const bool in = ae <= huber;
  const double w = in ? 1.0 : huber / ae;
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double wj = w * J[i];
#pragma unroll
    for (int j = i; j < 6; ++j) v[k++] = wj * J[j];
    v[21 + i] = wj * e;
  }
  v[27] = in ? (e * e) / 2.0 : huber * (ae - huber / 2.0);
  return true;
}

// exp(w) * R -> R: Rodrigues, the first-order form I + [w]x below theta^2 < 1e-16
RH_HD inline void rotate_left(const double* w, double* R) {
  const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
  double A = 1.0, B = 0.0;
  if (!(th2 < 1e-16)) {
    const double th = sqrt(th2);
    A = sin(th) / th;
    B = (1.0 - cos(th)) / th2;
  }
  const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  double E[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double kk = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
      E[3 * i + j] = ((i == j ? 1.0 : 0.0) + A * K[3 * i + j]) + B * kk;
    }
  double out[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) out[3 * i + j] = (E[3 * i] * R[j] + E[3 * i + 1] * R[3 + j]) + E[3 * i + 2] * R[6 + j];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = out[i];
}

// H d = -g by Cholesky (H = L L', column by column; H full, row-major). false: a pivot is not > 0 or not finite. ws: 42 doubles.
RH_HD inline bool solve6(const double* H, const double* g, double* ws, double* d) {
  double* L = ws;
  double* y = ws + 36;
  for (int j = 0; j < 6; ++j) {
    double s = H[6 * j + j];
    for (int k = 0; k < j; ++k) s = s - L[6 * j + k] * L[6 * j + k];
    if (!(s > 0.0 && s < HUGE_VAL)) return false;
    const double p = sqrt(s);
    L[6 * j + j] = p;
    for (int i = j + 1; i < 6; ++i) {
      double r = H[6 * i + j];
      for (int k = 0; k < j; ++k) r = r - L[6 * i + k] * L[6 * j + k];
      L[6 * i + j] = r / p;
    }
  }
  for (int i = 0; i < 6; ++i) {
    double r = -g[i];
    for (int k = 0; k < i; ++k) r = r - L[6 * i + k] * y[k];
    y[i] = r / L[6 * i + i];
  }
  for (int i = 5; i >= 0; --i) {
    double r = y[i];
    for (int k = i + 1; k < 6; ++k) r = r - L[6 * k + i] * d[k];
    d[i] = r / L[6 * i + i];
  }
  return true;
}

// One evaluation's end: S = the 28 sums (already added up in their fixed order), used = the terms behind them. Writes H, g, cost,
// used into *o; the first evaluation sets status 3 below min_used; unless this is the last evaluation (or a status stands) one
// Gauss-Newton step: status 2 and the pose left alone when H does not factor, t += d[0:3], R = exp(d[3:6]) R otherwise.
RH_HD inline void step(const double* S, int used, int first, int last, int min_used, double* ws, rebvio_hip_kf_pose* o) {
  for (int a = 0; a < 6; ++a) {
    for (int b = a; b < 6; ++b) o->H[6 * a + b] = o->H[6 * b + a] = S[h_index(a, b)];
    o->g[a] = S[21 + a];
  }
  o->cost = S[27];
  o->used = used;
  if (first && used < min_used) o->status = 3;
  if (last || o->status != 0) return;
  double* d = ws + 42;  // (ws: 48 doubles)
  if (!solve6(o->H, o->g, ws, d)) {
    o->status = 2;
    return;
  }
  for (int i = 0; i < 3; ++i) o->t[i] = o->t[i] + d[i];
  rotate_left(d + 3, o->R);
  o->iterations = o->iterations + 1;
}

}  // namespace kfp
}  // namespace rh
