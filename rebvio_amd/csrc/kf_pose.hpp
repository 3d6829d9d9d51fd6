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

// ---- alignment through the distance field (rebvio_hip_map_keyframe_align; include/rebvio_hip.h is the definition) ----------------
// What a term's lookup reads of the current map. The field either as the device keeps it (df: keys, decoded as k_df_decode does) or
// as rebvio_hip_map_distance_field hands it out (df null: ids with -1 for an empty cell, distances) - the host hook's form.
struct alignas(8) AlignF2 {  // one 8-byte load
  float x, y;
};
struct AlignMap {
  float fm, cx, cy;
  int rows, cols;
  const unsigned* df;
  int df_nr;
  const int* ids;
  const int* dists;
  const AlignF2* pos;   // KeyLine::pos
  const AlignF2* unit;  // gradient / gradient_norm
  int cap;              // slots of pos / unit: an id at or above it is skipped (detection's field holds none: the gathers stay inside)
};

// One term of the alignment: steps 2..6 of the definition for the keyframe keyline (kx, ky, rho_f; has_n: its normal knx, kny is
// there). -1: skipped, v untouched; otherwise the owning keyline i and v = the term's 28 addends.
RH_HD inline int align_term(const AlignMap& c, float kx, float ky, float rho_f, bool has_n, float knx, float kny, double min_cos,
                            int max_dist, const double* R, const double* t, double huber, double* v) {
  const double a = (double)(kx / c.fm), b = (double)(ky / c.fm), rho = (double)rho_f;
  const double Zx = (R[0] * a + R[1] * b) + R[2];
  const double Zy = (R[3] * a + R[4] * b) + R[5];
  const double Zz = (R[6] * a + R[7] * b) + R[8];
  const double Yx = Zx + rho * t[0], Yy = Zy + rho * t[1], Yz = Zz + rho * t[2];
  if (!(Yz > 0.0)) return -1;
  const double px = Yx / Yz, py = Yy / Yz;
  const double pu = (double)c.fm * px + (double)c.cx, pv = (double)c.fm * py + (double)c.cy;
  const double x = floor(pu + 0.5), y = floor(pv + 0.5);
  if (!(x >= 1.0 && x <= (double)(c.cols - 2) && y >= 1.0 && y <= (double)(c.rows - 2))) return -1;
  const size_t cell = (size_t)(int)y * (size_t)c.cols + (size_t)(int)x;
  int i, dist;
  if (c.df) {
    const unsigned key = c.df[cell];
    if (key == 0xFFFFFFFFu) return -1;  // (kDfEmpty)
    i = (int)((((1u << 23) - 1u) - (key & ((1u << 23) - 1u))) / (unsigned)c.df_nr);  // (kDfSeqMask, kDfSeqBits)
    dist = (int)(key >> 23);
  } else {
    i = c.ids[cell];
    dist = c.dists[cell];
    if (i < 0) return -1;
  }
  if (!(dist <= max_dist) || i >= c.cap) return -1;
  // pos[i] and unit[i]: two independent 8-byte gathers
  const AlignF2 ps = c.pos[i], un = c.unit[i];
  const float qx_f = ps.x - c.cx, qy_f = ps.y - c.cy;
  const float ux_f = un.x, uy_f = un.y;
  if (has_n && min_cos > -1.0) {
    const double nx = (double)knx, ny = (double)kny, ux = (double)ux_f, uy = (double)uy_f;
    const double mx = R[0] * nx + R[1] * ny, my = R[3] * nx + R[4] * ny;
    const double mm = mx * mx + my * my, nn = ux * ux + uy * uy;
    if (mm > 0.0 && nn > 0.0 && !(mx * ux + my * uy >= (min_cos * sqrt(mm)) * sqrt(nn))) return -1;
  }
  return term(c.fm, kx, ky, rho_f, qx_f, qy_f, ux_f, uy_f, R, t, huber, v) ? i : -1;
}

// ---- many hypotheses against one map (rebvio_hip_map_keyframe_align_many; include/rebvio_hip.h is the definition) ------------------
// term() and align_term(), copied statement for statement (the callers of the originals keep their instructions as they are), with
// one more output: *inlier = the term took the first branch of the Huber test, |e| <= huber. Written only when the term is used.
RH_HD inline bool term_in(float fm, float kx, float ky, float rho_f, float qx_f, float qy_f, float gx_f, float gy_f, const double* R,
                       const double* t, double huber, double* v, bool* inlier) {
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
  *inlier = in;
  return true;
}

RH_HD inline int align_term_in(const AlignMap& c, float kx, float ky, float rho_f, bool has_n, float knx, float kny, double min_cos,
                            int max_dist, const double* R, const double* t, double huber, double* v, bool* inlier) {
  const double a = (double)(kx / c.fm), b = (double)(ky / c.fm), rho = (double)rho_f;
  const double Zx = (R[0] * a + R[1] * b) + R[2];
  const double Zy = (R[3] * a + R[4] * b) + R[5];
  const double Zz = (R[6] * a + R[7] * b) + R[8];
  const double Yx = Zx + rho * t[0], Yy = Zy + rho * t[1], Yz = Zz + rho * t[2];
  if (!(Yz > 0.0)) return -1;
  const double px = Yx / Yz, py = Yy / Yz;
  const double pu = (double)c.fm * px + (double)c.cx, pv = (double)c.fm * py + (double)c.cy;
  const double x = floor(pu + 0.5), y = floor(pv + 0.5);
  if (!(x >= 1.0 && x <= (double)(c.cols - 2) && y >= 1.0 && y <= (double)(c.rows - 2))) return -1;
  const size_t cell = (size_t)(int)y * (size_t)c.cols + (size_t)(int)x;
  int i, dist;
  if (c.df) {
    const unsigned key = c.df[cell];
    if (key == 0xFFFFFFFFu) return -1;  // (kDfEmpty)
    i = (int)((((1u << 23) - 1u) - (key & ((1u << 23) - 1u))) / (unsigned)c.df_nr);  // (kDfSeqMask, kDfSeqBits)
    dist = (int)(key >> 23);
  } else {
    i = c.ids[cell];
    dist = c.dists[cell];
    if (i < 0) return -1;
  }
  if (!(dist <= max_dist) || i >= c.cap) return -1;
  // pos[i] and unit[i]: two independent 8-byte gathers
  const AlignF2 ps = c.pos[i], un = c.unit[i];
  const float qx_f = ps.x - c.cx, qy_f = ps.y - c.cy;
  const float ux_f = un.x, uy_f = un.y;
  if (has_n && min_cos > -1.0) {
    const double nx = (double)knx, ny = (double)kny, ux = (double)ux_f, uy = (double)uy_f;
    const double mx = R[0] * nx + R[1] * ny, my = R[3] * nx + R[4] * ny;
    const double mm = mx * mx + my * my, nn = ux * ux + uy * uy;
    if (mm > 0.0 && nn > 0.0 && !(mx * ux + my * uy >= (min_cos * sqrt(mm)) * sqrt(nn))) return -1;
  }
  return term_in(c.fm, kx, ky, rho_f, qx_f, qy_f, ux_f, uy_f, R, t, huber, v, inlier) ? i : -1;
}

// ---- depth fusion into a snapshot (rebvio_hip_kf_snapshot_fuse_depth; include/rebvio_hip.h is the definition) --------------------
constexpr float kRhoMin = 1e-3f;  // types/keyline.hpp:18: what the tracker clamps rho to (track.hip)
constexpr float kRhoMax = 20.0f;  // types/keyline.hpp:17

enum FuseOutcome { kFuseNone = 0, kFuseFused = 1, kFuseGated = 2, kFuseFlat = 3 };

// One keyframe keyline's scalar Kalman update: steps 2..7 of the definition (step 1, the filter, is the caller's). The lookup is
// align_term's, copied (a shared helper would have to leave every existing kernel's instructions as they are); e and c are the
// expressions of term(), without its Huber weight. kFuseNone: not associated, nothing written. Otherwise *owner = i, and for
// kFuseFused *rho_out / *sig_out = the new pair, *clamped = whether rho ran into kRhoMin / kRhoMax.
RH_HD inline int fuse_term(const AlignMap& c, float kx, float ky, float rho_f, float sig_f, bool has_n, float knx, float kny,
                           double min_cos, int max_dist, const double* R, const double* t, double pixel_sigma, double gate_sigma,
                           double q_abs, int* owner, float* rho_out, float* sig_out, bool* clamped) {
  const double a = (double)(kx / c.fm), b = (double)(ky / c.fm), rho = (double)rho_f;
  const double Zx = (R[0] * a + R[1] * b) + R[2];
  const double Zy = (R[3] * a + R[4] * b) + R[5];
  const double Zz = (R[6] * a + R[7] * b) + R[8];
  const double Yx = Zx + rho * t[0], Yy = Zy + rho * t[1], Yz = Zz + rho * t[2];
  if (!(Yz > 0.0)) return kFuseNone;
  const double px = Yx / Yz, py = Yy / Yz;
  const double pu = (double)c.fm * px + (double)c.cx, pv = (double)c.fm * py + (double)c.cy;
  const double x = floor(pu + 0.5), y = floor(pv + 0.5);
  if (!(x >= 1.0 && x <= (double)(c.cols - 2) && y >= 1.0 && y <= (double)(c.rows - 2))) return kFuseNone;
  const size_t cell = (size_t)(int)y * (size_t)c.cols + (size_t)(int)x;
  int i, dist;
  if (c.df) {
    const unsigned key = c.df[cell];
    if (key == 0xFFFFFFFFu) return kFuseNone;  // (kDfEmpty)
    i = (int)((((1u << 23) - 1u) - (key & ((1u << 23) - 1u))) / (unsigned)c.df_nr);  // (kDfSeqMask, kDfSeqBits)
    dist = (int)(key >> 23);
  } else {
    i = c.ids[cell];
    dist = c.dists[cell];
    if (i < 0) return kFuseNone;
  }
  if (!(dist <= max_dist) || i >= c.cap) return kFuseNone;
  // pos[i] and unit[i]: two independent 8-byte gathers
  const AlignF2 ps = c.pos[i], un = c.unit[i];
  const float qx_f = ps.x - c.cx, qy_f = ps.y - c.cy;
  if (has_n && min_cos > -1.0) {
    const double nx = (double)knx, ny = (double)kny, ux = (double)un.x, uy = (double)un.y;
    const double mx = R[0] * nx + R[1] * ny, my = R[3] * nx + R[4] * ny;
    const double mm = mx * mx + my * my, nn = ux * ux + uy * uy;
    if (mm > 0.0 && nn > 0.0 && !(mx * ux + my * uy >= (min_cos * sqrt(mm)) * sqrt(nn))) return kFuseNone;
  }
  // e and c of term()
  const double qx = (double)(qx_f / c.fm), qy = (double)(qy_f / c.fm);
  const double gx = (double)un.x, gy = (double)un.y;
  const double g2 = gx * gx + gy * gy;
  if (!(g2 > 0.0 && g2 < HUGE_VAL)) return kFuseNone;
  const double gn = sqrt(g2);
  const double nx = gx / gn, ny = gy / gn;
  const double f = (double)c.fm;
  const double e = f * (nx * (px - qx) + ny * (py - qy));
  const double cx = (f * nx) / Yz, cy = (f * ny) / Yz;
  const double cz = -(cx * px + cy * py);
  *owner = i;
  // the update: de/drho = c . t
  const double h = (cx * t[0] + cy * t[1]) + cz * t[2];
  const double s = (double)sig_f;
  const double v = s * s + q_abs * q_abs;
  const double hv = h * v;
  const double info = hv * h;
  if (!(info > 0.0)) return kFuseFlat;
  const double S = info + pixel_sigma * pixel_sigma;
  if (!(e * e <= (gate_sigma * gate_sigma) * S)) return kFuseGated;
  const double K = hv / S;
  double rho_n = rho - K * e;
  const double v_n = (1.0 - K * h) * v;
  double sig_n = sqrt(v_n);
  if (!(fabs(rho_n) < HUGE_VAL && v_n >= 0.0 && v_n < HUGE_VAL && fabs(sig_n) < HUGE_VAL)) return kFuseGated;
  const double lo = (double)kRhoMin, hi = (double)kRhoMax;
  *clamped = false;
  if (rho_n < lo) {
    sig_n = sig_n + (lo - rho_n);
    rho_n = lo;
    *clamped = true;
  } else if (rho_n > hi) {
    rho_n = hi;
    *clamped = true;
  }
  *rho_out = (float)rho_n;
  *sig_out = (float)sig_n;
  return kFuseFused;
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

// rotate_left, solve6 and step for k_kf_pose_step_many, copied statement for statement: a second device caller of the originals
// makes the compiler stop inlining them into k_kf_pose_step, whose instructions are to stay as they are. Device side only; the host
// uses the originals.
// exp(w) * R -> R: Rodrigues, the first-order form I + [w]x below theta^2 < 1e-16
RH_HD inline void rotate_left_m(const double* w, double* R) {
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
RH_HD inline bool solve6_m(const double* H, const double* g, double* ws, double* d) {
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
RH_HD inline void step_m(const double* S, int used, int first, int last, int min_used, double* ws, rebvio_hip_kf_pose* o) {
  for (int a = 0; a < 6; ++a) {
    for (int b = a; b < 6; ++b) o->H[6 * a + b] = o->H[6 * b + a] = S[h_index(a, b)];
    o->g[a] = S[21 + a];
  }
  o->cost = S[27];
  o->used = used;
  if (first && used < min_used) o->status = 3;
  if (last || o->status != 0) return;
  double* d = ws + 42;  // (ws: 48 doubles)
  if (!solve6_m(o->H, o->g, ws, d)) {
    o->status = 2;
    return;
  }
  for (int i = 0; i < 3; ++i) o->t[i] = o->t[i] + d[i];
  rotate_left_m(d + 3, o->R);
  o->iterations = o->iterations + 1;
}

}  // namespace kfp
}  // namespace rh
