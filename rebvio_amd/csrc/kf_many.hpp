// Many hypotheses against one map (rebvio_hip_map_keyframe_align_many; include/rebvio_hip.h is the definition): what of it runs on
// the host alone - the ranking of results, the 13 starts around a guess and the alignment loop of the host hooks. One source for the
// library (api.hip) and the stand-alone sanitizer program of tests/cpp, as kf_cloud.hpp does it. No device code here.
#pragma once

#include <cmath>
#include <cstring>

#include "kf_pose.hpp"
#include "rebvio_hip.h"

namespace rh {
namespace kfm {

// rebvio_hip_kf_align_best behind its argument check: status 0 and inliers >= min_inliers; the most inliers, then the smaller cost,
// then the lower index; -1: none
inline int best(const rebvio_hip_kf_hyp_result* res, int n, int min_inliers) {
  int b = -1;
  for (int h = 0; h < n; ++h) {
    if (res[h].pose.status != 0 || res[h].inliers < min_inliers) continue;
    if (b < 0 || res[h].inliers > res[b].inliers || (res[h].inliers == res[b].inliers && res[h].pose.cost < res[b].pose.cost)) b = h;
  }
  return b;
}

// rebvio_hip_kf_hypotheses_around behind its argument check (finite R, t, steps >= 0): out[0] = the guess, out[1..6] rotated by
// +- rot_step about x, y, z through kfp::rotate_left (the Gauss-Newton step's E), out[7..12] moved by +- trans_step along x, y, z
inline void around(rebvio_hip_kf_snapshot* snap, const double* R, const double* t, double rot_step, double trans_step,
                   rebvio_hip_kf_hypothesis* out) {
  for (int k = 0; k < 13; ++k) {
    out[k].snap = snap;
    for (int i = 0; i < 9; ++i) out[k].R0[i] = R[i];
    for (int i = 0; i < 3; ++i) out[k].t0[i] = t[i];
  }
  for (int a = 0; a < 3; ++a)
    for (int s = 0; s < 2; ++s) {
      double w[3] = {0.0, 0.0, 0.0};
      w[a] = s ? -rot_step : rot_step;
      kfp::rotate_left(w, out[1 + 2 * a + s].R0);
      out[7 + 2 * a + s].t0[a] = s ? t[a] - trans_step : t[a] + trans_step;
    }
}

// The alignment on the host, the loop of rebvio_hip_test_kf_align_host and of every hypothesis of
// rebvio_hip_test_kf_align_many_host: terms summed in index order from 0.0, one kfp::step per evaluation. o has been checked; a null
// R0 / t0 is the identity / zero. assoc (kf_size ints: the last evaluation's owners) and inliers (of the last evaluation, counted
// from the same term values) may be null.
inline void align_host(const kfp::AlignMap& am, const float* snap_prs4, const unsigned* snap_matches, const float* snap_normals,
                       int kf_size, const rebvio_hip_kf_align_opts& o, const double* R0, const double* t0, rebvio_hip_kf_pose* out,
                       int* assoc, int* inliers) {
  rebvio_hip_kf_pose res;
  std::memset(&res, 0, sizeof(res));
  for (int i = 0; i < 9; ++i) res.R[i] = R0 ? R0[i] : (i % 4 == 0 ? 1.0 : 0.0);
  for (int i = 0; i < 3; ++i) res.t[i] = t0 ? t0[i] : 0.0;
  res.candidates = kf_size;
  if (kf_size == 0) res.status = 3;
  int n_in = 0;
  for (int it = 0; kf_size > 0 && it <= o.max_iter; ++it) {
    double S[kfp::kSums] = {}, v[kfp::kSums], ws[48];
    int used = 0;
    n_in = 0;
    for (int j = 0; j < kf_size; ++j) {
      const float* k4 = snap_prs4 + 4 * (size_t)j;
      int i = -1;
      bool in = false;
      if (kfp::filter_pass(o.kf_filter, k4[2], k4[3], snap_matches[j]))
        i = kfp::align_term(am, k4[0], k4[1], k4[2], snap_normals != nullptr, snap_normals ? snap_normals[2 * (size_t)j] : 0.0f,
                            snap_normals ? snap_normals[2 * (size_t)j + 1] : 0.0f, o.min_cos, o.max_dist, res.R, res.t, o.huber_px, v, &in);
      if (assoc) assoc[j] = i;
      if (i < 0) continue;
      for (int k = 0; k < kfp::kSums; ++k) S[k] = S[k] + v[k];
      ++used;
      if (in) ++n_in;
    }
    kfp::step(S, used, it == 0, it == o.max_iter, o.min_used, ws, &res);
  }
  *out = res;
  if (inliers) *inliers = n_in;
}

}  // namespace kfm
}  // namespace rh
