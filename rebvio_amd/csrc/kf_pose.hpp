// Keyframe-to-current pose (rebvio_hip_map_keyframe_pose; include/rebvio_hip.h is the definition): the term of one correspondence
// and the O(1) math of one Gauss-Newton step - 6x6 Cholesky solve, SE3 update - and what the solvers built on it add: the lookup
// through a map's distance field (alignment, many hypotheses, depth fusion, hand-over) and the fusion's scalar update. Every
// statement stands here once. One source for the device (the k_kf_* kernels, track.hip) and the host (the
// rebvio_hip_test_kf_*_host hooks, api.hip), as glue.hpp / hostmath.hpp do it. fp64 throughout; every + - * / and sqrt is an
// operation of its own (-ffp-contract=off), so a result's bits follow from the order written inside each expression alone.
#pragma once

#include "hostmath.hpp"  // RH_HD
#include "rebvio_hip.h"

// On the device every function below is inlined into its kernel, whatever the number of callers: the kernels are straight-line
// code around one statement each, and the compiler's own choice changes with the number of call sites (two callers of step() made
// it a function of 1637 instructions).
#if defined(__HIP_DEVICE_COMPILE__)
#define RH_KF __host__ __device__ __attribute__((always_inline)) inline
#else
#define RH_KF RH_HD inline
#endif

namespace rh {
namespace kfp {

constexpr int kSums = 28;  // 21 unique w J_a J_b (a <= b, row-major), 6 w J_a e, the cost

// index of H(a, b), a <= b, among the 21
RH_HD inline int h_index(int a, int b) { return a * 6 - a * (a - 1) / 2 + (b - a); }

// the test of cloud_pass (track.hip) on the keyframe side of a correspondence
RH_HD inline bool filter_pass(const rebvio_hip_cloud_filter& f, float rho, float sigma_rho, unsigned matches) {
  return matches >= f.min_matches && rho >= f.rho_min && rho <= f.rho_max && sigma_rho <= f.max_rel_sigma * rho;
}

// The keyframe keyline (kx, ky, rho: pos_img and rho of the snapshot) under the pose (R, t): Z = R (a, b, 1), Y = Z + rho t,
// (px, py) = Y / Yz. false: Yz is not > 0 (a NaN fails), px / py unset.
struct Proj {
  double rho, Zx, Zy, Zz, Yz, px, py;
};
RH_KF bool project(float fm, float kx, float ky, float rho_f, const double* R, const double* t, Proj* o) {
  const double a = (double)(kx / fm), b = (double)(ky / fm), rho = (double)rho_f;
  const double Zx = (R[0] * a + R[1] * b) + R[2];
  const double Zy = (R[3] * a + R[4] * b) + R[5];
  const double Zz = (R[6] * a + R[7] * b) + R[8];
  const double Yx = Zx + rho * t[0], Yy = Zy + rho * t[1], Yz = Zz + rho * t[2];
  o->rho = rho;
  o->Zx = Zx;
  o->Zy = Zy;
  o->Zz = Zz;
  o->Yz = Yz;
  if (!(Yz > 0.0)) return false;
  o->px = Yx / Yz;
  o->py = Yy / Yz;
  return true;
}

// The direction (nx, ny) of a gradient (gx, gy). false: the gradient is zero, NaN or infinite.
RH_KF bool direction(float gx_f, float gy_f, double* nx, double* ny) {
  const double gx = (double)gx_f, gy = (double)gy_f;
  const double g2 = gx * gx + gy * gy;
  if (!(g2 > 0.0 && g2 < HUGE_VAL)) return false;
  const double gn = sqrt(g2);
  *nx = gx / gn;
  *ny = gy / gn;
  return true;
}

// The residual of a projected keyline against the current keyline (qx, qy: pos_img; gx, gy: gradient): e in pixels along the
// gradient's direction, and c = de/dY. false: the gradient has no direction.
RH_KF bool residual(float fm, const Proj& p, float qx_f, float qy_f, float gx_f, float gy_f, double* e, double* c) {
  const double qx = (double)(qx_f / fm), qy = (double)(qy_f / fm);
  double nx, ny;
  if (!direction(gx_f, gy_f, &nx, &ny)) return false;
  const double f = (double)fm;
  *e = f * (nx * (p.px - qx) + ny * (p.py - qy));
  const double cx = (f * nx) / p.Yz, cy = (f * ny) / p.Yz;
  c[0] = cx;
  c[1] = cy;
  c[2] = -(cx * p.px + cy * p.py);
  return true;
}

// The 28 addends of a projected keyline's term. false: skipped, v and *inlier untouched. *inlier = the term took the first branch
// of the Huber test, |e| <= huber.
RH_KF bool term_at(float fm, const Proj& p, float qx_f, float qy_f, float gx_f, float gy_f, double huber, double* v, bool* inlier) {
  double e, c[3];
  if (!residual(fm, p, qx_f, qy_f, gx_f, gy_f, &e, c)) return false;
  const double cx = c[0], cy = c[1], cz = c[2];
  double J[6];
  J[0] = p.rho * cx;
  J[1] = p.rho * cy;
  J[2] = p.rho * cz;
  J[3] = p.Zy * cz - p.Zz * cy;
  J[4] = p.Zz * cx - p.Zx * cz;
  J[5] = p.Zx * cy - p.Zy * cx;
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

// One term: the keyframe keyline (kx, ky, rho) seen as the current keyline (qx, qy: pos_img; gx, gy: gradient) under the pose
// (R, t). false: skipped (positive tests, a NaN skips), v and *inlier untouched. true: v = the term's 28 addends. A caller with no
// use for *inlier passes a dummy.
RH_KF bool term(float fm, float kx, float ky, float rho_f, float qx_f, float qy_f, float gx_f, float gy_f, const double* R,
                const double* t, double huber, double* v, bool* inlier) {
  Proj p;
  return project(fm, kx, ky, rho_f, R, t, &p) && term_at(fm, p, qx_f, qy_f, gx_f, gy_f, huber, v, inlier);
}

// ---- the lookup through a map's distance field (rebvio_hip_map_keyframe_align; include/rebvio_hip.h is the definition) -----------
// What a lookup reads of the current map. The field either as the device keeps it (df: keys, decoded as k_df_decode does) or as
// rebvio_hip_map_distance_field hands it out (df null: ids with -1 for an empty cell, distances) - the host hooks' form.
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

// the host hooks' AlignMap: the field as ids and distances, pos / unit as n_cur pairs of floats
inline AlignMap host_map(float fm, float cx, float cy, int rows, int cols, const int* ids, const int* dists, const float* pos,
                         const float* unit, int n_cur) {
  AlignMap am;
  am.fm = fm; am.cx = cx; am.cy = cy; am.rows = rows; am.cols = cols;
  am.df = nullptr; am.df_nr = 1; am.ids = ids; am.dists = dists;
  am.pos = reinterpret_cast<const AlignF2*>(pos); am.unit = reinterpret_cast<const AlignF2*>(unit);
  am.cap = n_cur;
  return am;
}

// What the lookup of one keyframe keyline finds: its projection, the owning keyline i of the cell it lands in, the owner's
// gradient direction (ux, uy) and - kPos - the owner's pos less the principal point (qx, qy).
struct Lookup {
  Proj p;
  int owner;
  float qx, qy, ux, uy;
};

// Steps 2..5 of the alignment's definition for the keyframe keyline (kx, ky, rho_f; has_n: its normal knx, kny is there): project,
// cell, owner, gradient-direction test. false: not associated. kPos: pos[i] is loaded next to unit[i] - two independent 8-byte
// gathers behind the field's; without it unit[i] alone (pos[i] serves the residual only).
template <bool kPos>
RH_KF bool lookup(const AlignMap& c, float kx, float ky, float rho_f, bool has_n, float knx, float kny, double min_cos, int max_dist,
                  const double* R, const double* t, Lookup* o) {
  if (!project(c.fm, kx, ky, rho_f, R, t, &o->p)) return false;
  const double px = o->p.px, py = o->p.py;
  const double pu = (double)c.fm * px + (double)c.cx, pv = (double)c.fm * py + (double)c.cy;
  const double x = floor(pu + 0.5), y = floor(pv + 0.5);
  if (!(x >= 1.0 && x <= (double)(c.cols - 2) && y >= 1.0 && y <= (double)(c.rows - 2))) return false;
  const size_t cell = (size_t)(int)y * (size_t)c.cols + (size_t)(int)x;
  int i, dist;
  if (c.df) {
    const unsigned key = c.df[cell];
    if (key == 0xFFFFFFFFu) return false;  // (kDfEmpty)
    i = (int)((((1u << 23) - 1u) - (key & ((1u << 23) - 1u))) / (unsigned)c.df_nr);  // (kDfSeqMask, kDfSeqBits)
    dist = (int)(key >> 23);
  } else {
    i = c.ids[cell];
    dist = c.dists[cell];
    if (i < 0) return false;
  }
  if (!(dist <= max_dist) || i >= c.cap) return false;
  if (kPos) {
    const AlignF2 ps = c.pos[i], un = c.unit[i];
    o->qx = ps.x - c.cx;
    o->qy = ps.y - c.cy;
    o->ux = un.x;
    o->uy = un.y;
  } else {
    const AlignF2 un = c.unit[i];
    o->ux = un.x;
    o->uy = un.y;
  }
  if (has_n && min_cos > -1.0) {
    const double nx = (double)knx, ny = (double)kny, ux = (double)o->ux, uy = (double)o->uy;
    const double mx = R[0] * nx + R[1] * ny, my = R[3] * nx + R[4] * ny;
    const double mm = mx * mx + my * my, nn = ux * ux + uy * uy;
    if (mm > 0.0 && nn > 0.0 && !(mx * ux + my * uy >= (min_cos * sqrt(mm)) * sqrt(nn))) return false;
  }
  o->owner = i;
  return true;
}

// One term of the alignment: steps 2..6 of the definition. -1: skipped, v and *inlier untouched; otherwise the owning keyline i,
// v = the term's 28 addends and *inlier as term() leaves it.
RH_KF int align_term(const AlignMap& c, float kx, float ky, float rho_f, bool has_n, float knx, float kny, double min_cos, int max_dist,
                     const double* R, const double* t, double huber, double* v, bool* inlier) {
  Lookup l;
  if (!lookup<true>(c, kx, ky, rho_f, has_n, knx, kny, min_cos, max_dist, R, t, &l)) return -1;
  return term_at(c.fm, l.p, l.qx, l.qy, l.ux, l.uy, huber, v, inlier) ? l.owner : -1;
}

// ---- depth fusion into a snapshot (rebvio_hip_kf_snapshot_fuse_depth; include/rebvio_hip.h is the definition) --------------------
constexpr float kRhoMin = 1e-3f;  // types/keyline.hpp:18: what the tracker clamps rho to (track.hip)
constexpr float kRhoMax = 20.0f;  // types/keyline.hpp:17

enum FuseOutcome { kFuseNone = 0, kFuseFused = 1, kFuseGated = 2, kFuseFlat = 3 };

// One keyframe keyline's scalar Kalman update: steps 2..7 of the definition (step 1, the filter, is the caller's): lookup(), then
// e and c of residual() - the term's, without its Huber weight. kFuseNone: not associated, nothing written. Otherwise *owner = i,
// and for kFuseFused *rho_out / *sig_out = the new pair, *clamped = whether rho ran into kRhoMin / kRhoMax.
RH_KF int fuse_term(const AlignMap& c, float kx, float ky, float rho_f, float sig_f, bool has_n, float knx, float kny, double min_cos,
                    int max_dist, const double* R, const double* t, double pixel_sigma, double gate_sigma, double q_abs, int* owner,
                    float* rho_out, float* sig_out, bool* clamped) {
  Lookup l;
  if (!lookup<true>(c, kx, ky, rho_f, has_n, knx, kny, min_cos, max_dist, R, t, &l)) return kFuseNone;
  double e, cc[3];
  if (!residual(c.fm, l.p, l.qx, l.qy, l.ux, l.uy, &e, cc)) return kFuseNone;
  const double cx = cc[0], cy = cc[1], cz = cc[2], rho = l.p.rho;
  *owner = l.owner;
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

// ---- one Gauss-Newton step ----------------------------------------------------------------------------------------------------------
// exp(w) * R -> R: Rodrigues, the first-order form I + [w]x below theta^2 < 1e-16
RH_KF void rotate_left(const double* w, double* R) {
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
RH_KF bool solve6(const double* H, const double* g, double* ws, double* d) {
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
RH_KF void step(const double* S, int used, int first, int last, int min_used, double* ws, rebvio_hip_kf_pose* o) {
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
