// Depth hand-over from a retiring keyframe snapshot to its successor (rebvio_hip_kf_snapshot_handover_depth; include/rebvio_hip.h
// is the definition): the two per-keyline statements, and the two passes over them in index order. One source for the device
// (k_kf_handover_claim / k_kf_handover_apply, track.hip) and the host (handover_host: rebvio_hip_test_kf_handover_host, api.hip, and
// the stand-alone tests/cpp/kf_handover_host_check.cpp). fp64 behind the loads; every
// + - * / and sqrt is an operation of its own (-ffp-contract=off). The lookup is kfp::lookup (kf_pose.hpp), the alignment's and the
// fusion's as well.
#pragma once

#include "kf_pose.hpp"  // AlignMap, lookup, direction, filter_pass, kRhoMin / kRhoMax

namespace rh {
namespace kfp {

enum HandoverOutcome { kHoNone = 0, kHoOutOfRange = 1, kHoClaim = 2 };      // of the claim pass, per src keyline
enum HandoverSlot { kHoEmpty = 0, kHoAdopted = 1, kHoKept = 2, kHoConflict = 3 };  // of the apply pass, per dst keyline

constexpr unsigned long long kHoEmptyKey = 0xFFFFFFFFFFFFFFFFull;  // a slot nobody claimed (no claimant's key: j < 2^32 - 1)

// What a claimant leaves for the apply pass besides its key (which carries the bits of (float)sig_c): one 8-byte record.
struct alignas(8) HandoverStage {
  float rho_c;
  unsigned matches;
};

RH_HD inline unsigned long long handover_key(float sig_c, int j) {
  union {
    float f;
    unsigned u;
  } b;
  b.f = sig_c;  // sig_c >= +0 and not NaN (handover_claim_term): the bits order as the values do
  return ((unsigned long long)b.u << 32) | (unsigned long long)(unsigned)j;
}

RH_HD inline float handover_key_sigma(unsigned long long key) {
  union {
    float f;
    unsigned u;
  } b;
  b.u = (unsigned)(key >> 32);
  return b.f;
}

// Pass 1 for one src keyline that passed the filter (the caller's test): steps 1..3 of the definition. kHoNone: not associated,
// nothing written. Otherwise *owner = i < dst_size; kHoClaim: *rho_out / *sig_out = (float)rho_c / (float)sig_c.
RH_KF int handover_claim_term(const AlignMap& c, int dst_size, float kx, float ky, float rho_f, float sig_f, bool has_n, float knx, float kny,
                             double min_cos, int max_dist, const double* R, const double* t, double q_abs, int* owner, float* rho_out,
                             float* sig_out) {
  Lookup l;
  if (!lookup<false>(c, kx, ky, rho_f, has_n, knx, kny, min_cos, max_dist, R, t, &l)) return kHoNone;
  // step 6's own skip: the owner's gradient
  double nx, ny;
  if (!direction(l.ux, l.uy, &nx, &ny)) return kHoNone;
  const int i = l.owner;
  const double rho = l.p.rho, Zz = l.p.Zz, Yz = l.p.Yz;
  if (!(i < dst_size)) return kHoNone;  // the successor has no such keyline
  *owner = i;
  // 2. propagate into the map's frame
  const double rho_c = rho / Yz;
  const double d = Zz / (Yz * Yz);
  const double s = (double)sig_f;
  const double sig_c = fabs(d) * sqrt(s * s + q_abs * q_abs);
  const double lo = (double)kRhoMin, hi = (double)kRhoMax;
  if (!(fabs(rho_c) < HUGE_VAL && fabs(sig_c) < HUGE_VAL && sig_c >= 0.0 && rho_c >= lo && rho_c <= hi)) return kHoOutOfRange;
  *rho_out = (float)rho_c;
  *sig_out = (float)sig_c;
  return kHoClaim;
}

// Pass 2 for one claimed dst keyline: steps 4..5. (rc, sc, mj) = the winner's staged values, (rho_i, sig_i, mi) = the slot's.
// kHoAdopted: the slot gets rc, sc and *matches_out; otherwise it keeps all its bits.
RH_HD inline int handover_apply_term(float rc, float sc, unsigned mj, float rho_i, float sig_i, unsigned mi, double gate_sigma,
                                     unsigned* matches_out) {
  const double dr = (double)rc - (double)rho_i;
  const double bound = (gate_sigma * gate_sigma) * ((double)sc * (double)sc + (double)sig_i * (double)sig_i);
  if (!(dr * dr <= bound)) return kHoConflict;
  if (!(sc < sig_i)) return kHoKept;
  *matches_out = mi > mj ? mi : mj;
  return kHoAdopted;
}

// The whole hand-over on the host, both passes in index order (rebvio_hip_test_kf_handover_host; arguments checked by the caller).
// Scratch of the caller: key = dst_size words, stage = kf_size records, assoc = kf_size ints (the output as well).
inline void handover_host(const AlignMap& am, const float* src_prs4, const unsigned* src_matches, const float* src_normals, int kf_size,
                          float* dst_prs4, unsigned* dst_matches, int dst_size, const rebvio_hip_kf_handover_opts& o, const double* R,
                          const double* t, unsigned long long* key, HandoverStage* stage, int* assoc, rebvio_hip_kf_handover* out) {
  rebvio_hip_kf_handover res = {};
  res.candidates = kf_size;
  for (int i = 0; i < dst_size; ++i) key[i] = kHoEmptyKey;
  for (int j = 0; j < kf_size; ++j) {  // pass 1
    const float* k4 = src_prs4 + 4 * (size_t)j;
    int outcome = kHoNone, i = 0;
    float rho_c = 0.f, sig_c = 0.f;
    if (filter_pass(o.kf_filter, k4[2], k4[3], src_matches[j]))
      outcome = handover_claim_term(am, dst_size, k4[0], k4[1], k4[2], k4[3], src_normals != nullptr,
                                    src_normals ? src_normals[2 * (size_t)j] : 0.0f, src_normals ? src_normals[2 * (size_t)j + 1] : 0.0f,
                                    o.min_cos, o.max_dist, R, t, o.q_abs, &i, &rho_c, &sig_c);
    assoc[j] = outcome == kHoNone ? -2147483647 - 1 : -1 - i;
    stage[j] = HandoverStage{0.f, 0u};
    if (outcome == kHoNone) continue;
    ++res.associated;
    if (outcome == kHoOutOfRange) {
      ++res.out_of_range;
      continue;
    }
    stage[j] = HandoverStage{rho_c, src_matches[j]};
    const unsigned long long k = handover_key(sig_c, j);
    if (k < key[i]) key[i] = k;
  }
  for (int i = 0; i < dst_size; ++i) {  // pass 2
    const unsigned long long k = key[i];
    if (k == kHoEmptyKey) continue;
    const int win = (int)(unsigned)k;
    float* d4 = dst_prs4 + 4 * (size_t)i;
    const float sc = handover_key_sigma(k);
    unsigned mt_n = dst_matches[i];
    const int slot = handover_apply_term(stage[win].rho_c, sc, stage[win].matches, d4[2], d4[3], dst_matches[i], o.gate_sigma, &mt_n);
    ++res.claimed;
    if (slot == kHoConflict) ++res.conflicts;
    if (slot == kHoKept) ++res.kept;
    if (slot != kHoAdopted) continue;
    ++res.adopted;
    d4[2] = stage[win].rho_c;
    d4[3] = sc;
    dst_matches[i] = mt_n;
    assoc[win] = i;
  }
  *out = res;
}

}  // namespace kfp
}  // namespace rh
