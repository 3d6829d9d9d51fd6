// The depth prior a rectified stereo partner gives a map's keylines: EdgeMap::fuseStereo, Rebvio::rightImageCallback. No reference
// counterpart; include/rebvio_hip.h ("Depth prior from a rectified stereo partner") defines every term. StereoPriorOpts and
// StereoPriorCounts are layout-compatible with the C-ABI's rebvio_hip_stereo_prior_opts / _counts.
#pragma once

namespace rebvio {
namespace types {

struct StereoPriorOpts {
  double baseline{0.0};          // > 0, no default: metres from the left camera to the right one along the left camera's x axis
  double d_min{0.0};             // 0 <= d_min <= d_max <= cols: accepted disparities, pixels
  double d_max{64.0};
  double min_ux{0.5};            // in (0, 1]: least |x component| of a unit gradient, left and right
  int row_tol{1};                // 0 or 1: rows searched above and below the keyline's
  double sigma_px{0.5};          // > 0: standard deviation of a disparity along the gradient, pixels
  double gate_sigma{3.0};        // > 0: innovation gate in standard deviations
  double ambig_px{2.0};          // >= 0: largest spread of the disparities inside the gate
  double cos_min{(double)0.70710677f};  // (float)cos(45 deg): least cosine between the two gradients (the tracker's match_threshold_angle: 45 degrees)
  double norm_tol{1.0};          // largest |gn' / gn - 1| (the tracker's match_threshold_norm)
  double q_abs{0.0};             // >= 0: added in quadrature to sigma_rho before the update
  int reserved{0};
};
static_assert(sizeof(StereoPriorOpts) == 96, "StereoPriorOpts must stay layout-compatible with rebvio_hip_stereo_prior_opts");

// seen = fused + gated + ambiguous
struct StereoPriorCounts {
  int candidates{0};  // the left map's size
  int usable{0};      // keylines whose edge is not too parallel to the epipolar line
  int seen{0};        // ... with at least one candidate in the window
  int fused{0};       // ... updated
  int gated{0};       // ... no candidate inside the gate, or a non-finite update (left as they were)
  int ambiguous{0};   // ... the gate's candidates spread over more than ambig_px (left as they were)
  int clamped{0};     // among fused: rho ran into RHO_MIN or RHO_MAX
  int reserved{0};
};
static_assert(sizeof(StereoPriorCounts) == 32, "StereoPriorCounts must stay layout-compatible with rebvio_hip_stereo_prior_counts");

}  // namespace types
}  // namespace rebvio
