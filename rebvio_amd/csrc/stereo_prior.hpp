// Depth prior from a rectified stereo partner's edge map (rebvio_hip_map_fuse_stereo*; include/rebvio_hip.h is the definition): the
// per-keyline statements - direction and search window of a left keyline, the test of one right keyline met in the window, the
// fold of the candidates and one scalar Kalman update of (rho, sigma_rho). One source for the device (k_stereo_prior, track.hip)
// and the host (rebvio_hip_test_stereo_prior_host, api.hip), as depth_prior.hpp does it. fp64 behind the loads; every + - * / sqrt,
// floor and ceil is an operation of its own (-ffp-contract=off). Only minima, maxima, an OR and the smallest (score, j) are folded
// over a keyline's candidates, so the order in which the window's cells are visited - by one host loop or by the lanes of a
// sub-group - does not show in any output bit.
#pragma once

#include <math.h>
#include <stdint.h>

#include "kf_pose.hpp"  // RH_KF, kRhoMin / kRhoMax
#include "rebvio_hip.h"

namespace rh {
namespace spr {

enum Outcome { kNone = 0, kFused = 1, kGated = 2, kUnusable = 3, kAmbiguous = 4, kClampedBit = 32 };

// The geometry and the options as a kernel takes them by value (SGPRs). fb = fm * baseline, formed once.
struct Args {
  int rows, cols, row_tol;
  int c_lo, c_hi;  // the window's columns relative to xi: xi - c_lo ... xi - c_hi (before clipping)
  double fb, d_min, d_max, min_ux, sigma_px, gate2, ambig_px, cos_min, norm_tol, q2;
};

inline Args make_args(int rows, int cols, float fm, const rebvio_hip_stereo_prior_opts& o) {
  Args a;
  a.rows = rows;
  a.cols = cols;
  a.row_tol = o.row_tol;
  a.c_lo = (int)ceil(o.d_max) + 1;
  a.c_hi = (int)floor(o.d_min) - 1;
  a.fb = (double)fm * o.baseline;
  a.d_min = o.d_min;
  a.d_max = o.d_max;
  a.min_ux = o.min_ux;
  a.sigma_px = o.sigma_px;
  a.gate2 = o.gate_sigma * o.gate_sigma;
  a.ambig_px = o.ambig_px;
  a.cos_min = o.cos_min;
  a.norm_tol = o.norm_tol;
  a.q2 = o.q_abs * o.q_abs;
  return a;
}

// Steps 1, 2 and the keyline's own part of step 4 for one left keyline.
struct Left {
  double px, py, gx, gy, gn, rho, v, S;
  int x0, x1, yi;  // the window's columns, clipped (x0 > x1: clipped to nothing), and its centre row
};

// kUnusable, kNone (no window at all) or -1: the window is to be searched.
RH_KF int left_setup(const Args& a, float px_f, float py_f, float gx_f, float gy_f, float gn_f, float rho_f, float sig_f, Left* L) {
  const bool gpos = gn_f > 0.0f;
  const double ux = gpos ? (double)gx_f / (double)gn_f : 0.0, uy = gpos ? (double)gy_f / (double)gn_f : 0.0;
  if (!(gpos && fabs(ux) < HUGE_VAL && fabs(uy) < HUGE_VAL && fabs(ux) >= a.min_ux)) return kUnusable;
  L->px = (double)px_f;
  L->py = (double)py_f;
  const double xh = L->px + 0.5, yh = L->py + 0.5;
  if (!(xh >= 0.0 && xh < (double)a.cols && yh >= 0.0 && yh < (double)a.rows)) return kNone;
  const int xi = (int)floor(xh);
  L->yi = (int)floor(yh);
  const int x0 = xi - a.c_lo, x1 = xi - a.c_hi;
  L->x0 = x0 < 0 ? 0 : x0;
  L->x1 = x1 > a.cols - 1 ? a.cols - 1 : x1;
  L->gx = (double)gx_f;
  L->gy = (double)gy_f;
  L->gn = (double)gn_f;
  L->rho = (double)rho_f;
  const double s = (double)sig_f;
  L->v = s * s + a.q2;
  const double s_m = (a.sigma_px / fabs(ux)) / a.fb;
  L->S = L->v + s_m * s_m;
  return -1;
}

// What a keyline's candidates fold into. seen: bit 0 a candidate, bit 1 one inside the gate.
struct Fold {
  int seen;
  double d_lo, d_hi, score, d_win;  // (score, j, d_win): the best in-gate candidate so far
  int j;
};
RH_KF void fold_clear(Fold* f) {
  f->seen = 0;
  f->d_lo = HUGE_VAL;
  f->d_hi = -HUGE_VAL;
  f->score = HUGE_VAL;
  f->d_win = 0.0;
  f->j = 0x7fffffff;
}
RH_KF void fold_join(Fold* f, const Fold& o) {
  f->seen |= o.seen;
  if (o.d_lo < f->d_lo) f->d_lo = o.d_lo;
  if (o.d_hi > f->d_hi) f->d_hi = o.d_hi;
  if (o.score < f->score || (o.score == f->score && o.j < f->j)) {
    f->score = o.score;
    f->d_win = o.d_win;
    f->j = o.j;
  }
}

// Step 3 and the gate of step 4 for the right keyline j: false when it is no candidate; else *d is its disparity and *in_gate
// whether its innovation passes.
RH_KF bool candidate(const Args& a, const Left& L, float qx_f, float qy_f, float hx_f, float hy_f, float hn_f, double* d_out, bool* in_gate,
                     double* score) {
  const double hn = (double)hn_f, hx = (double)hx_f, hy = (double)hy_f;
  if (!(hn > 0.0)) return false;
  const double dot = L.gx * hx + L.gy * hy;
  if (!(dot / (L.gn * hn) >= a.cos_min)) return false;
  if (!(fabs(hn / L.gn - 1.0) <= a.norm_tol)) return false;
  const double uxr = hx / hn, uyr = hy / hn;
  if (!(fabs(uxr) >= a.min_ux)) return false;
  const double xr = (double)qx_f - (uyr * (L.py - (double)qy_f)) / uxr;
  const double d = L.px - xr;
  if (!(d > 0.0 && a.d_min <= d && d <= a.d_max)) return false;
  const double rho_m = d / a.fb;
  const double e = rho_m - L.rho;
  *in_gate = e * e <= a.gate2 * L.S;
  const double ex = L.gx - hx, ey = L.gy - hy;
  *score = ex * ex + ey * ey;
  *d_out = d;
  return true;
}

// One cell's keyline folded into f (steps 3 and 4).
RH_KF void fold_candidate(const Args& a, const Left& L, int j, float qx_f, float qy_f, float hx_f, float hy_f, float hn_f, Fold* f) {
  double d, score;
  bool in_gate;
  if (!candidate(a, L, qx_f, qy_f, hx_f, hy_f, hn_f, &d, &in_gate, &score)) return;
  Fold o;
  fold_clear(&o);
  o.seen = 1;
  if (in_gate) {
    o.seen = 3;
    o.d_lo = o.d_hi = d;
    o.score = score;
    o.d_win = d;
    o.j = j;
  }
  fold_join(f, o);
}

// Steps 4 (GATED), 5 and the decision of 6 once the window is folded: kNone, kGated, kAmbiguous or -1: f.j is the winner, f.d_win its
// disparity.
RH_KF int decide(const Args& a, const Fold& f) {
  if (!(f.seen & 1)) return kNone;
  if (!(f.seen & 2)) return kGated;
  if (f.d_hi - f.d_lo > a.ambig_px) return kAmbiguous;
  return -1;
}

// Step 6 with the winner's disparity d. kFused (+ kClampedBit) with the new pair, or kGated for a non-finite update.
RH_KF int update(const Args& a, const Left& L, double d, float* rho_out, float* sig_out) {
  const double rho_m = d / a.fb;
  const double e = rho_m - L.rho;
  const double K = L.v / L.S;
  double rho_n = L.rho + K * e;
  const double v_n = (1.0 - K) * L.v;
  double sig_n = sqrt(v_n);
  if (!(fabs(rho_n) < HUGE_VAL && v_n >= 0.0 && v_n < HUGE_VAL && fabs(sig_n) < HUGE_VAL)) return kGated;
  int flags = 0;
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

}  // namespace spr
}  // namespace rh
