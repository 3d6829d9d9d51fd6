// Straight line segments of a map's edge polylines (rebvio_hip_map_edge_segments; include/rebvio_hip.h is the definition): the
// per-point statements of every step - the squared deviation and its key, what a winner's key decides, the kept test, one member of
// the depth fit, the fit's end - and the steps over them in point order. One source for the device (k_seg_*, track.hip) and the
// host (segments_host: rebvio_hip_test_edge_segments_host, api.hip, and the stand-alone tests/cpp/edge_segments_host_check.cpp), as
// edge_chains.hpp does it. fp32 for the image-plane geometry, fp64 for the fit; every * / + - an operation of its own
// (-ffp-contract=off), so a result's bits follow from the order written inside each expression alone.
#pragma once

#include <math.h>
#include <string.h>

#include "edge_chains.hpp"  // RH_HD, ech::poly_xyz: the point of an end
#include "rebvio_hip.h"

namespace rh {
namespace esg {

// Launches of the segment step behind the polylines' R + 8, whatever the map holds: k_seg_init, max_rounds x (k_seg_far +
// k_seg_split), the measuring k_seg_far, k_seg_count, k_seg_emit, k_seg_fit.
RH_HD inline int seg_launches(int max_rounds) { return 2 * max_rounds + 5; }
constexpr int kMaxRounds = 32;
// words of the device: [0] points [1] lines [2] segments_all [3] kept [4] depth_valid [5] unresolved
// [8 + k] "something split in front of round k" (k = 0 .. max_rounds; [8] = 1)
constexpr int kSegWords = 8 + kMaxRounds + 8;
constexpr int kLanes = 16;  // partial sums of the fit = lanes of its row

// One point as the steps read it: pos_img, rho, sigma_rho of its keyline.
struct alignas(16) SegPoint {
  float x, y, rho, sigma;
};
// One point's state: interior to [a, b] (a < p < b) or a vertex (a == b == p).
struct alignas(8) SegSpan {
  int a, b;
};

RH_HD inline unsigned f32_bits(float f) {
  unsigned u;
  memcpy(&u, &f, 4);
  return u;
}
RH_HD inline float bits_f32(unsigned u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

RH_HD inline float seg_l2(const SegPoint& qa, const SegPoint& qb) {
  const float ex = qb.x - qa.x, ey = qb.y - qa.y;
  return ex * ex + ey * ey;
}

// squared distance of point qp from the line through qa and qb (from qa when the two coincide); a NaN gives 0
RH_HD inline float seg_dev2(const SegPoint& qa, const SegPoint& qb, const SegPoint& qp) {
  const float ex = qb.x - qa.x, ey = qb.y - qa.y, px = qp.x - qa.x, py = qp.y - qa.y;
  const float l2 = ex * ex + ey * ey, cr = ex * py - ey * px;
  float d2 = (l2 == 0.0f) ? px * px + py * py : (cr * cr) / l2;
  if (!(d2 >= 0.0f)) d2 = 0.0f;
  return d2;
}

// the key of interior point p: the largest d2 wins, a tie goes to the lowest p (d2 >= 0: its bits order as it does)
RH_HD inline unsigned long long seg_key(float d2, int p) {
  return ((unsigned long long)f32_bits(d2) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)p);
}
RH_HD inline float key_dev2(unsigned long long key) { return bits_f32((unsigned)(key >> 32)); }
RH_HD inline int key_point(unsigned long long key) { return (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)); }
// a segment's winner splits it; 0 = the key of a segment without an interior point
RH_HD inline bool key_splits(unsigned long long key, float tol2) { return key != 0ull && key_dev2(key) > tol2; }

// What one split round makes of interior point p with span s, from its segment's winner key. *won: p is the winner (it then
// stores nxt[a] = p and nxt[p] = b).
RH_HD inline SegSpan seg_split(SegSpan s, int p, unsigned long long key, float tol2, bool* won) {
  *won = false;
  if (!key_splits(key, tol2)) return s;
  const int m = key_point(key);
  if (p == m) {
    *won = true;
    return SegSpan{p, p};
  }
  if (p < m) s.b = m; else s.a = m;
  return s;
}

RH_HD inline bool seg_kept(int points, float l2, int min_points, float min_len2) { return points >= min_points && l2 >= min_len2; }

// the six sums of the fit: Sw, Swt, Swtt, Swr, Swtr, Swrr
struct FitSums {
  double s[6];
};
RH_HD inline FitSums fit_zero() { return FitSums{{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}}; }
// one member of segment [qa, qb] (l2 = seg_l2 of the two) added to a partial
RH_HD inline void fit_add(FitSums* f, const SegPoint& qa, const SegPoint& qb, float l2, const SegPoint& qp) {
  const float ex = qb.x - qa.x, ey = qb.y - qa.y, px = qp.x - qa.x, py = qp.y - qa.y;
  const float tf = (px * ex + py * ey) / l2;
  float sg = fabsf(qp.sigma);
  if (!(sg >= 1e-6f)) sg = 1e-6f;
  const double w = 1.0 / ((double)sg * (double)sg);
  const double t = (double)tf, r = (double)qp.rho;
  const double wt = w * t, wr = w * r;
  f->s[0] = f->s[0] + w;
  f->s[1] = f->s[1] + wt;
  f->s[2] = f->s[2] + wt * t;
  f->s[3] = f->s[3] + wr;
  f->s[4] = f->s[4] + wt * r;
  f->s[5] = f->s[5] + wr * r;
}
RH_HD inline FitSums fit_pair(const FitSums& x, const FitSums& y) {
  FitSums o;
#pragma unroll
  for (int k = 0; k < 6; ++k) o.s[k] = x.s[k] + y.s[k];
  return o;
}

// The record of a kept segment from its sums. first_point = a, points = b - a + 1.
RH_HD inline rebvio_hip_line_segment fit_finish(const FitSums& f, const SegPoint& qa, const SegPoint& qb, float max_dev2, int a, int points,
                                                int line, bool unresolved, float fm, const float* R, const float* t, float scale,
                                                float rho_min, float rho_max) {
  const double Sw = f.s[0], Swt = f.s[1], Swtt = f.s[2], Swr = f.s[3], Swtr = f.s[4], Swrr = f.s[5];
  const double det = Sw * Swtt - Swt * Swt;
  const double r0 = (Swtt * Swr - Swt * Swtr) / det;
  const double sl = (Sw * Swtr - Swt * Swr) / det;
  const double r1 = r0 + sl;
  const double v0 = Swtt / det;
  const double v1 = ((Swtt - 2.0 * Swt) + Sw) / det;
  double chi2 = Swrr - (r0 * Swr + sl * Swtr);
  if (!(chi2 > 0.0)) chi2 = 0.0;
  const float rho0 = (float)r0, rho1 = (float)r1;
  const bool valid = det > 0.0 && v0 >= 0.0 && v1 >= 0.0 && rho0 >= rho_min && rho0 <= rho_max && rho1 >= rho_min && rho1 <= rho_max;
  rebvio_hip_line_segment s;
  for (int k = 0; k < 3; ++k) s.xyz0[k] = s.xyz1[k] = 0.0f;
  s.rho0 = s.rho1 = s.sigma_rho0 = s.sigma_rho1 = 0.0f;
  if (valid) {
    ech::poly_xyz(fm, R, t, scale, qa.x, qa.y, rho0, s.xyz0);
    ech::poly_xyz(fm, R, t, scale, qb.x, qb.y, rho1, s.xyz1);
    s.rho0 = rho0;
    s.rho1 = rho1;
    s.sigma_rho0 = (float)sqrt(v0);
    s.sigma_rho1 = (float)sqrt(v1);
  }
  s.uv0[0] = qa.x; s.uv0[1] = qa.y;
  s.uv1[0] = qb.x; s.uv1[1] = qb.y;
  s.max_dev2 = max_dev2;
  s.chi2 = (float)chi2;
  s.first_point = a;
  s.points = points;
  s.line = line;
  s.flags = (valid ? 1 : 0) | (unresolved ? 2 : 0);
  return s;
}

// The segments of np points in nl lines on the host, every step in point order. q = np points; lines = nl records of the
// polylines (first_point, points). Scratch of the caller: span = np, nxt = np ints, far = np keys. min(kept, cap) records are
// written; the counts are of everything.
inline void segments_host(float fm, const SegPoint* q, int np, const rebvio_hip_polyline* lines, int nl, const rebvio_hip_segment_opts& o,
                          const float* R, const float* t, float scale, SegSpan* span, int* nxt, int* line_of, unsigned long long* far,
                          rebvio_hip_line_segment* segs, int cap, rebvio_hip_segment_counts* counts) {
  const float tol2 = o.tol * o.tol, min_len2 = o.min_length * o.min_length;
  for (int l = 0; l < nl; ++l) {  // init
    const int first = lines[l].first_point, last = first + lines[l].points - 1;
    for (int p = first; p <= last; ++p) {
      const bool vertex = p == first || p == last;
      span[p] = vertex ? SegSpan{p, p} : SegSpan{first, last};
      nxt[p] = p == first ? last : p;  // the line's last point begins nothing (a line of one point: first == last)
      line_of[p] = l;
    }
  }
  auto measure = [&]() {  // far[a] of every segment
    for (int p = 0; p < np; ++p) far[p] = 0ull;
    for (int p = 0; p < np; ++p) {
      const SegSpan s = span[p];
      if (s.a == p) continue;
      const unsigned long long key = seg_key(seg_dev2(q[s.a], q[s.b], q[p]), p);
      if (key > far[s.a]) far[s.a] = key;
    }
  };
  int rounds_used = 0;
  for (int k = 0; k < o.max_rounds; ++k) {  // rounds (one that follows a round in which nothing split does nothing)
    measure();
    bool moved = false;
    for (int p = 0; p < np; ++p) {
      const SegSpan s = span[p];
      if (s.a == p) continue;
      bool won;
      span[p] = seg_split(s, p, far[s.a], tol2, &won);
      if (won) {
        nxt[s.a] = p;
        nxt[p] = s.b;
        moved = true;
      }
    }
    if (!moved) break;
    ++rounds_used;
  }
  measure();  // (after a round without a split this repeats that round's measure)
  int all = 0, kept = 0, valid = 0, unresolved = 0;
  for (int a = 0; a < np; ++a) {  // count + emit + fit
    if (span[a].a != a || nxt[a] == a) continue;
    const int b = nxt[a], points = b - a + 1;
    const bool unres = key_splits(far[a], tol2);
    ++all;
    unresolved += unres;
    const float l2 = seg_l2(q[a], q[b]);
    if (!seg_kept(points, l2, o.min_points, min_len2)) continue;
    FitSums part[kLanes];
    for (int j = 0; j < kLanes; ++j) {
      part[j] = fit_zero();
      for (int i = j; i < points; i += kLanes) fit_add(&part[j], q[a], q[b], l2, q[a + i]);
    }
    for (int w = 1; w < kLanes; w <<= 1)
      for (int j = 0; j < kLanes; j += 2 * w) part[j] = fit_pair(part[j], part[j + w]);
    const rebvio_hip_line_segment rec = fit_finish(part[0], q[a], q[b], key_dev2(far[a]), a, points, line_of[a], unres, fm, R, t, scale,
                                                   o.poly.filter.rho_min, o.poly.filter.rho_max);
    valid += rec.flags & 1;
    if (kept < cap) segs[kept] = rec;
    ++kept;
  }
  counts->segments_all = all;
  counts->kept = kept;
  counts->depth_valid = valid;
  counts->unresolved = unresolved;
  counts->rounds_used = rounds_used;
  counts->points = np;
  counts->lines = nl;
  counts->reserved = 0;
}

}  // namespace esg
}  // namespace rh
