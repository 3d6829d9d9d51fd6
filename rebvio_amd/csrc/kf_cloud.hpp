// Point cloud of a keyframe snapshot (rebvio_hip_kf_snapshot_point_cloud; include/rebvio_hip.h is the definition): the per-record
// statement - filter and position of one snapshot keyline. One source for the device (k_kf_cloud_count / k_kf_cloud_emit,
// track.hip) and the host (rebvio_hip_test_kf_cloud_host, api.hip), as kf_pose.hpp does it. fp32 throughout; every * / + is an
// operation of its own (-ffp-contract=off). k_cloud_emit (a map's cloud) keeps its own copy of the same statement.
#pragma once

#include "kf_pose.hpp"  // RH_HD, kfp::filter_pass: the filter, as the pose, the alignment and the fusion apply it to a snapshot's keylines
#include "rebvio_hip.h"

namespace rh {
namespace kfc {

// One snapshot keyline (px, py: pos_img; rho, sigma_rho, matches as stored): false when the filter drops it (xyz untouched), else
// xyz = R * ((px / fm, py / fm, 1) * (scale / rho)) + t in the operation order of k_cloud_emit.
RH_HD inline bool record(float fm, const rebvio_hip_cloud_filter& f, const float* R, const float* t, float scale, float px, float py,
                         float rho, float sigma_rho, unsigned matches, float* xyz) {
  if (!kfp::filter_pass(f, rho, sigma_rho, matches)) return false;
  const float u = px / fm, v = py / fm;
  const float z = scale / rho;
  const float xc = u * z, yc = v * z;
#pragma unroll
  for (int i = 0; i < 3; ++i) xyz[i] = ((R[3 * i] * xc + R[3 * i + 1] * yc) + R[3 * i + 2] * z) + t[i];
  return true;
}

// The whole cloud on the host, in index order: *count = keylines that pass, min(count, cap) records written (the hook, and the
// stand-alone sanitizer program of tests/cpp).
inline void extract_host(float fm, const float* prs4, const unsigned* matches, int n, const rebvio_hip_cloud_filter& f, const float* R,
                         const float* t, float scale, rebvio_hip_cloud_point* points, int cap, int* count) {
  int k = 0;
  for (int j = 0; j < n; ++j) {
    const float* p = prs4 + 4 * (size_t)j;
    float q[3];
    if (!record(fm, f, R, t, scale, p[0], p[1], p[2], p[3], matches[j], q)) continue;
    if (k < cap) {
      rebvio_hip_cloud_point& o = points[k];
      o.xyz[0] = q[0];
      o.xyz[1] = q[1];
      o.xyz[2] = q[2];
      o.rho = p[2];
      o.sigma_rho = p[3];
      o.gradient_norm = 0.0f;  // the snapshot does not keep it
      o.keyline = j;
      o.matches = matches[j];
    }
    ++k;
  }
  *count = k;
}

}  // namespace kfc
}  // namespace rh
