// Depth prior from a registered depth image (rebvio_hip_map_fuse_depth_image*; include/rebvio_hip.h is the definition): the
// per-keyline statement - three taps along the gradient, the nearer surface as the measurement, one scalar Kalman update of
// (rho, sigma_rho). One source for the device (k_depth_prior, track.hip) and the host (rebvio_hip_test_depth_prior_host, api.hip),
// as kf_pose.hpp does it. fp64 behind the loads; every + - * / sqrt and floor is an operation of its own (-ffp-contract=off), so a
// result's bits follow from the order written inside each expression alone.
#pragma once

#include <math.h>
#include <stdint.h>

#include "kf_pose.hpp"  // RH_KF, kRhoMin / kRhoMax
#include "rebvio_hip.h"

namespace rh {
namespace dpr {

enum Outcome { kNone = 0, kFused = 1, kGated = 2, kJumpBit = 16, kClampedBit = 32 };

// The image and the options as a kernel takes them by value (SGPRs).
struct Args {
  const void* img;  // rows x cols taps of 2 (U16) or 4 (F32) bytes, `pitch` bytes from row to row
  long long pitch;
  int rows, cols, fmt;
  double tap_px, jump_rel, z_min, z_max, sigma_z0, sigma_z2, gate_sigma, q_abs, unit;
};

inline Args make_args(const void* img, size_t pitch, int rows, int cols, int fmt, const rebvio_hip_depth_prior_opts& o) {
  Args a;
  a.img = img;
  a.pitch = (long long)pitch;
  a.rows = rows;
  a.cols = cols;
  a.fmt = fmt;
  a.tap_px = o.tap_px;
  a.jump_rel = o.jump_rel;
  a.z_min = o.z_min;
  a.z_max = o.z_max;
  a.sigma_z0 = o.sigma_z0;
  a.sigma_z2 = o.sigma_z2;
  a.gate_sigma = o.gate_sigma;
  a.q_abs = o.q_abs;
  a.unit = o.unit;
  return a;
}

// One tap at (x, y): false when it lies outside the image or its depth is invalid (positive tests: a NaN fails them).
RH_KF bool tap(const Args& a, double x, double y, double* z_out) {
  const double xh = x + 0.5, yh = y + 0.5;
  if (!(xh >= 0.0 && xh < (double)a.cols && yh >= 0.0 && yh < (double)a.rows)) return false;
  const int xi = (int)floor(xh), yi = (int)floor(yh);
  const char* row = static_cast<const char*>(a.img) + (long long)yi * a.pitch;
  double z;
  if (a.fmt == REBVIO_HIP_DEPTH_U16) {
    const uint16_t v = reinterpret_cast<const uint16_t*>(row)[xi];
    if (v == 0) return false;
    z = (double)v * a.unit;
  } else {
    z = (double)reinterpret_cast<const float*>(row)[xi];
  }
  if (!(a.z_min <= z && z <= a.z_max)) return false;
  *z_out = z;
  return true;
}

// Steps 1..6 of the definition for one keyline. Returns the outcome word; for kFused *rho_out / *sig_out are the new pair,
// otherwise they are not written.
RH_KF int term(const Args& a, float px_f, float py_f, float gx_f, float gy_f, float gn_f, float rho_f, float sig_f, float* rho_out,
               float* sig_out) {
  const double px = (double)px_f, py = (double)py_f;
  const bool gpos = gn_f > 0.0f;
  const double ux = gpos ? (double)gx_f / (double)gn_f : 0.0, uy = gpos ? (double)gy_f / (double)gn_f : 0.0;
  const bool dir = gpos && fabs(ux) < HUGE_VAL && fabs(uy) < HUGE_VAL;
  double z_near = 0.0, z_far = 0.0, z;
  bool any = tap(a, px, py, &z);
  if (any) z_near = z_far = z;
  if (dir) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const double s = k == 0 ? 1.0 : -1.0;
      const double d = s * a.tap_px;
      if (tap(a, px + d * ux, py + d * uy, &z)) {
        if (!any) {
          z_near = z_far = z;
          any = true;
        } else {
          if (z < z_near) z_near = z;
          if (z > z_far) z_far = z;
        }
      }
    }
  }
  if (!any) return kNone;
  int flags = 0;
  if (z_far - z_near > a.jump_rel * z_near) flags |= kJumpBit;
  const double rho_m = 1.0 / z_near;
  const double s_m = (a.sigma_z0 * rho_m) * rho_m + a.sigma_z2;
  const double rho = (double)rho_f;
  const double s = (double)sig_f;
  const double v = s * s + a.q_abs * a.q_abs;
  const double e = rho_m - rho;
  const double S = v + s_m * s_m;
  if (!(e * e <= (a.gate_sigma * a.gate_sigma) * S)) return kGated | flags;
  const double K = v / S;
  double rho_n = rho + K * e;
  const double v_n = (1.0 - K) * v;
  double sig_n = sqrt(v_n);
  if (!(fabs(rho_n) < HUGE_VAL && v_n >= 0.0 && v_n < HUGE_VAL && fabs(sig_n) < HUGE_VAL)) return kGated | flags;
  const double lo = (double)kfp::kRhoMin, hi = (double)kfp::kRhoMax;
  if (rho_n < lo) {
    sig_n = sig_n + (lo - rho_n);
    rho_n = lo;
    flags |= kClampedBit;
  } else if (rho_n > hi) {
    rho_n = hi;
    flags |= kClampedBit;
  }
  *rho_out = (float)rho_n;
  *sig_out = (float)sig_n;
  return kFused | flags;
}

}  // namespace dpr
}  // namespace rh
