// Edge chains and polylines of a map (rebvio_hip_map_edge_chains / rebvio_hip_map_edge_polylines; include/rebvio_hip.h is the
// definition): the per-keyline statements of every step - link, one pointer-jumping round, resolve, kept / begin / end of a slot, the
// point - and the steps over them in index order. One source for the device (k_chain_* / k_poly_*, track.hip) and the host
// (chains_host / polylines_host: rebvio_hip_test_edge_chains_host / _edge_polylines_host, api.hip, and the stand-alone
// tests/cpp/edge_chains_host_check.cpp), as kf_handover.hpp does it. Integers throughout but for the point, whose statement is
// k_cloud_emit's (fp32, every * / + an operation of its own: -ffp-contract=off).
#pragma once

#include "kf_pose.hpp"  // RH_HD, kfp::filter_pass: the test of cloud_pass
#include "rebvio_hip.h"

namespace rh {
namespace ech {

// State of one keyline between two rounds: anc = the keyline reached after d pred steps, m = the smallest index among the d
// keylines of those steps (this one first, anc not among them), dm = the number of steps to m's first occurrence. A head (no pred)
// has d = 0 and anc = itself; every other keyline has d >= 1.
struct alignas(16) ChainNode {
  int anc, d, m, dm;
};

// rounds after which every path member has reached its head and every cycle member has been round its cycle: 2^rounds >= cap
RH_HD inline int chain_rounds(int cap) {
  int r = 0;
  while ((1 << r) < cap) ++r;
  return r;
}

// succ(i) / pred(j) of the definition. No value outside 0..n-1 is used as an index.
RH_HD inline int chain_succ(const int* id_prev, const int* id_next, int n, int i) {
  const int s = id_next[i];
  if (s < 0 || s >= n || s == i) return -1;
  return id_prev[s] == i ? s : -1;
}
RH_HD inline int chain_pred(const int* id_prev, const int* id_next, int n, int j) {
  // succ(i) == j asks for id_prev[j] == i: the only candidate is id_prev[j]
  const int p = id_prev[j];
  if (p < 0 || p >= n || p == j) return -1;
  return id_next[p] == j ? p : -1;
}

RH_HD inline ChainNode chain_init(int i, int pred) { return pred < 0 ? ChainNode{i, 0, i, 0} : ChainNode{pred, 1, i, 0}; }

// One round for keyline i over the previous round's states. A path member doubles its span until its ancestor is the head
// (d < n always: a rank is at most n - 1); a cycle member until its span has been round the cycle (d >= n).
RH_HD inline ChainNode chain_round(const ChainNode* prev, int i, int n, bool* moved) {
  ChainNode s = prev[i];
  if (s.d == 0 || s.d >= n) return s;
  const ChainNode a = prev[s.anc];
  if (a.d == 0) return s;  // anc is a head
  if (a.m < s.m) {
    s.m = a.m;
    s.dm = s.d + a.dm;
  }
  s.d += a.d;
  s.anc = a.anc;
  *moved = true;
  return s;
}

// After the last round: head, rank and "cyclic" of keyline i.
RH_HD inline void chain_resolve(const ChainNode* st, int i, int* head, int* rank, int* cyclic) {
  const ChainNode s = st[i];
  if (s.d == 0) {
    *head = i; *rank = 0; *cyclic = 0;
  } else if (st[s.anc].d == 0) {
    *head = s.anc; *rank = s.d; *cyclic = 0;
  } else {
    *head = s.m; *rank = s.dm; *cyclic = 1;
  }
}

// the one member of a chain that stores its length (rank + 1): a path's tail, a cycle's member in front of the head
RH_HD inline bool chain_is_last(int succ, int head) { return succ < 0 || succ == head; }

// Polylines: a slot's keyline is kept when it passes the cloud filter and its chain is long enough.
RH_HD inline bool poly_kept(const rebvio_hip_cloud_filter& f, int min_chain_length, float rho, float sigma_rho, unsigned matches,
                            int length) {
  return kfp::filter_pass(f, rho, sigma_rho, matches) && length >= min_chain_length;
}

// the point of one kept keyline: the statement of k_cloud_emit
RH_HD inline void poly_xyz(float fm, const float* R, const float* t, float scale, float px, float py, float rho, float* xyz) {
  const float u = px / fm, v = py / fm;
  const float z = scale / rho;
  const float xc = u * z, yc = v * z;
#pragma unroll
  for (int i = 0; i < 3; ++i) xyz[i] = ((R[3 * i] * xc + R[3 * i + 1] * yc) + R[3 * i + 2] * z) + t[i];
}

// what the emit step leaves in a line record for the last step: first_point, the index behind the line's last point in `points`,
// head, and the chain's length in `flags` when the chain is cyclic (0 otherwise)
RH_HD inline void poly_line_finish(rebvio_hip_polyline* l) {
  const int pts = l->points - l->first_point;
  l->flags = (l->flags != 0 && pts == l->flags) ? 1 : 0;
  l->points = pts;
}

// The chains of n keylines on the host, every step in index order. Scratch of the caller: a, b = n nodes each, succ / len /
// start_of = n ints each. Outputs in full: refs = n records, order = n ints, starts = n + 1 ints (C + 1 used), *n_chains = C.
inline void chains_host(const int* id_prev, const int* id_next, int n, ChainNode* a, ChainNode* b, int* succ, int* len, int* start_of,
                        rebvio_hip_chain_ref* refs, int* order, int* starts, int* n_chains) {
  for (int i = 0; i < n; ++i) {  // link
    succ[i] = chain_succ(id_prev, id_next, n, i);
    a[i] = chain_init(i, chain_pred(id_prev, id_next, n, i));
  }
  const int rounds = chain_rounds(n);
  ChainNode* in = a;
  ChainNode* out = b;
  bool moved = true;
  for (int k = 0; k < rounds; ++k) {  // rounds (one that follows a round in which nothing moved returns at once)
    if (!moved) break;
    moved = false;
    for (int i = 0; i < n; ++i) out[i] = chain_round(in, i, n, &moved);
    ChainNode* x = in;
    in = out;
    out = x;
  }
  for (int i = 0; i < n; ++i) {  // rank
    int head, rank, cyc;
    chain_resolve(in, i, &head, &rank, &cyc);
    refs[i].head = head;
    refs[i].rank = rank;
    refs[i].length = 0;
    refs[i].flags = cyc;
    if (chain_is_last(succ[i], head)) len[head] = rank + 1;
  }
  int c = 0, start = 0;
  for (int i = 0; i < n; ++i) {  // count + emit: chain numbers and starts by ascending head
    refs[i].length = len[refs[i].head];
    if (refs[i].head != i) continue;
    starts[c++] = start;
    start_of[i] = start;
    start += refs[i].length;
  }
  starts[c] = n;
  *n_chains = c;
  for (int i = 0; i < n; ++i) {  // order
    const int slot = start_of[refs[i].head] + refs[i].rank;
    if (slot >= 0 && slot < n) order[slot] = i;
  }
}

// The polylines of n keylines on the host from the chain table, slot by slot. pos_img / rs = n pairs (rs: rho, sigma_rho).
// *n_points / *n_lines = all of them; min(n_points, cap_points) points (and refs2 entries, refs2 may be null) and
// min(n_lines, cap_lines) lines are written. A line's first_point counts every point, written or not.
inline void polylines_host(float fm, const float* pos_img, const float* rs, const float* gnorm, const unsigned* matches, int n,
                           const rebvio_hip_chain_ref* refs, const int* order, const rebvio_hip_polyline_opts& o, const float* R,
                           const float* t, float scale, rebvio_hip_cloud_point* points, int* refs2, int cap_points,
                           rebvio_hip_polyline* lines, int cap_lines, int* n_points, int* n_lines) {
  int np = 0, nl = 0;
  bool prev_kept = false;
  for (int s = 0; s < n; ++s) {
    const int k = order[s];
    const rebvio_hip_chain_ref ref = refs[k];
    const bool kept = poly_kept(o.filter, o.min_chain_length, rs[2 * (size_t)k], rs[2 * (size_t)k + 1], matches[k], ref.length);
    const bool begin = kept && (ref.rank == 0 || !prev_kept);
    bool next_kept = false;
    if (ref.rank + 1 < ref.length) {
      const int k2 = order[s + 1];
      next_kept = poly_kept(o.filter, o.min_chain_length, rs[2 * (size_t)k2], rs[2 * (size_t)k2 + 1], matches[k2], ref.length);
    }
    const bool end = kept && !next_kept;
    if (begin) {
      if (nl < cap_lines) {
        lines[nl].first_point = np;
        lines[nl].head = ref.head;
        lines[nl].flags = (ref.flags & 1) ? ref.length : 0;
      }
      ++nl;
    }
    if (kept) {
      if (np < cap_points) {
        rebvio_hip_cloud_point& p = points[np];
        poly_xyz(fm, R, t, scale, pos_img[2 * (size_t)k], pos_img[2 * (size_t)k + 1], rs[2 * (size_t)k], p.xyz);
        p.rho = rs[2 * (size_t)k];
        p.sigma_rho = rs[2 * (size_t)k + 1];
        p.gradient_norm = gnorm[k];
        p.keyline = k;
        p.matches = matches[k];
        if (refs2) {
          refs2[2 * (size_t)np] = ref.head;
          refs2[2 * (size_t)np + 1] = ref.rank;
        }
      }
      ++np;
    }
    if (end && nl - 1 < cap_lines) {
      lines[nl - 1].points = np;
      poly_line_finish(&lines[nl - 1]);
    }
    prev_kept = kept;
  }
  *n_points = np;
  *n_lines = nl;
}

}  // namespace ech
}  // namespace rh
