// Registered depth images (RGB-D) and the depth prior they give a map's keylines: EdgeMap::fuseDepthImage,
// Rebvio::depthImageCallback. No reference counterpart; include/rebvio_hip.h ("Depth prior from a registered depth image") defines
// every term. DepthPriorOpts and DepthPriorCounts are layout-compatible with the C-ABI's rebvio_hip_depth_prior_opts / _counts.
#pragma once

#include <cstddef>
#include <cstdint>

namespace rebvio {
namespace types {

enum DepthFormat : int {
  DEPTH_U16 = 0,  // uint16 counts of `unit` metres, 0 = invalid (REBVIO_HIP_DEPTH_U16)
  DEPTH_F32 = 1   // float metres (REBVIO_HIP_DEPTH_F32)
};

// A stamped depth image in the geometry of the image the detector sees (with a lens model: the undistorted one), depth along the
// optical axis. `data` is not owned: it has to stay valid for the call it is handed to (Rebvio::depthImageCallback copies it).
struct DepthImage {
  const void* data{nullptr};
  int rows{0}, cols{0};
  size_t pitch{0};     // bytes from row to row; 0 = dense
  int format{DEPTH_U16};
  double unit{0.0};    // metres per count of a DEPTH_U16 image; 0 = the options' unit (default 0.001)
  uint64_t ts_us{0};   // the stamp of the camera frame it belongs to
};
static_assert(sizeof(DepthImage) == 48, "DepthImage: pointer, two ints, pitch, format, unit, stamp");

struct DepthPriorOpts {
  double tap_px{2.0};      // >= 0: distance of the two side taps along the gradient, pixels
  double jump_rel{0.1};    // >= 0: a keyline sits on a depth jump when z_far - z_near > jump_rel * z_near
  double z_min{0.1};       // > 0, metres
  double z_max{20.0};      // >= z_min
  double sigma_z0{1e-3};   // >= 0: the sensor's sigma_z = sigma_z0 + sigma_z2 * z^2
  double sigma_z2{2e-3};   // >= 0; sigma_z0 + sigma_z2 > 0
  double gate_sigma{3.0};  // > 0: innovation gate in standard deviations
  double q_abs{0.0};       // >= 0: added in quadrature to sigma_rho before the update
  double unit{0.001};      // > 0: metres per count of a DEPTH_U16 image
  int reserved{0};
};
static_assert(sizeof(DepthPriorOpts) == 80, "DepthPriorOpts must stay layout-compatible with rebvio_hip_depth_prior_opts");

// sampled = fused + gated
struct DepthPriorCounts {
  int candidates{0};  // the map's size
  int sampled{0};     // keylines with at least one valid tap
  int fused{0};       // ... updated
  int gated{0};       // ... failed the innovation gate or gave a non-finite update (left as they were)
  int jumps{0};       // among sampled: on a depth jump (the nearer surface was taken)
  int clamped{0};     // among fused: rho ran into RHO_MIN or RHO_MAX
};
static_assert(sizeof(DepthPriorCounts) == 24, "DepthPriorCounts must stay layout-compatible with rebvio_hip_depth_prior_counts");

}  // namespace types
}  // namespace rebvio
