// Point cloud of an edge map's depth-bearing keylines (no reference counterpart: the reference hands out poses, edge images
// and whole maps only). Records, filter and pose are layout-compatible with the C-ABI's rebvio_hip_cloud_point / _filter / _pose;
// rebvio_hip.h defines the filter and the position of a point exactly.
#pragma once

#include <cstddef>
#include <cstdint>

namespace rebvio {
class KeyframeSnapshot;  // edge_map.hpp
namespace types {

struct CloudPoint {
  float xyz[3];          // pose.R * (pos_img / fm, 1) * pose.scale / rho + pose.t
  float rho;             // KeyLine::rho
  float sigma_rho;       // KeyLine::sigma_rho
  float gradient_norm;   // KeyLine::gradient_norm ("intensity" of a sensor_msgs/PointCloud2)
  int keyline;           // index of the source keyline in its map; strictly increasing within a cloud
  unsigned int matches;  // KeyLine::matches
};
static_assert(sizeof(CloudPoint) == 32, "CloudPoint must stay layout-compatible with rebvio_hip_cloud_point");

// A keyline passes when matches >= min_matches, rho_min <= rho <= rho_max and sigma_rho <= max_rel_sigma * rho.
// The defaults are rebvio_hip_default_cloud_filter's.
struct CloudFilter {
  unsigned int min_matches{2};
  float max_rel_sigma{0.5f};
  float rho_min{1e-3f};
  float rho_max{20.0f};
};

struct CloudPose {
  float R[9]{1, 0, 0, 0, 1, 0, 0, 0, 1};  // row-major
  float t[3]{0, 0, 0};
  float scale{1.0f};
};

// One keyframe-to-current correspondence (EdgeMap::keyframeMatches; layout-compatible with the C-ABI's rebvio_hip_kf_match, which
// defines claimants and winner exactly): keyline `kf_keyline` of the keyframe map lives on in this map as keyline `keyline`.
struct KfMatch {
  int kf_keyline;        // index in the keyframe map; strictly increasing within a result
  int keyline;           // index in this map of the winning claimant (smallest sigma_rho, smallest index among equals)
  int claimants;         // keylines of this map whose match_id_keyframe is kf_keyline
  unsigned int matches;  // winner's KeyLine::matches
  float rho, sigma_rho;  // winner's
  float pos_img[2];      // winner's
};
static_assert(sizeof(KfMatch) == 32, "KfMatch must stay layout-compatible with rebvio_hip_kf_match");

// Options and result of EdgeMap::keyframePose, layout-compatible with the C-ABI's rebvio_hip_kf_pose_opts / rebvio_hip_kf_pose
// (rebvio_hip.h defines every term of the estimate). The defaults are rebvio_hip_default_kf_pose_opts's.
struct KfPoseOpts {
  CloudFilter kf_filter;  // applied to the keyframe side of a correspondence
  double huber_px{2.0};
  int max_iter{8};        // 0..32; 0: the sums at the guess only
  int min_used{12};
};
static_assert(sizeof(KfPoseOpts) == 32, "KfPoseOpts must stay layout-compatible with rebvio_hip_kf_pose_opts");
struct KfPose {
  double R[9]{1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3]{0, 0, 0};  // X_cur = R X_kf + t, in keyframe depth units (1 / rho)
  double H[36]{}, g[6]{}, cost{0};                        // J' W J, J' W e and the Huber cost at that pose
  int candidates{0}, used{0}, iterations{0};
  int status{0};  // 0 ok, 2 H not positive definite, 3 fewer than min_used terms at the first evaluation
};
static_assert(sizeof(KfPose) == 55 * 8 + 16, "KfPose must stay layout-compatible with rebvio_hip_kf_pose");

// Options of EdgeMap::keyframeAlign, layout-compatible with the C-ABI's rebvio_hip_kf_align_opts (rebvio_hip.h defines every term). The
// defaults are rebvio_hip_default_kf_align_opts's; max_dist -1 stands for the context's search_range (EdgeMap::keyframeAlign fills it in).
struct KfAlignOpts {
  CloudFilter kf_filter;  // applied to the keyframe keylines
  double huber_px{2.0};
  double min_cos{0.9};    // the gradient test, where the snapshot has a non-zero normal; -1 disables it
  int max_dist{-1};       // 0..search_range cells between the projection and the keyline that owns its cell
  int max_iter{8};        // 0..32; 0: the sums at the guess only
  int min_used{12};
};
static_assert(sizeof(KfAlignOpts) == 48, "KfAlignOpts must stay layout-compatible with rebvio_hip_kf_align_opts");

// One hypothesis and one result of EdgeMap::keyframeAlignMany, laid out like the C-ABI's rebvio_hip_kf_hypothesis /
// rebvio_hip_kf_hyp_result (rebvio_hip.h defines every term): a snapshot (which the caller keeps alive) and the guess to start from;
// the pose EdgeMap::keyframeAlign returns for the same snapshot, guess and options, bit for bit, and the number of used terms with
// |e| <= huber_px at that pose.
struct KfHypothesis {
  const rebvio::KeyframeSnapshot* snapshot{nullptr};
  double R0[9]{1, 0, 0, 0, 1, 0, 0, 0, 1}, t0[3]{0, 0, 0};
};
static_assert(sizeof(KfHypothesis) == 104 && offsetof(KfHypothesis, R0) == 8 && offsetof(KfHypothesis, t0) == 80,
              "KfHypothesis must stay laid out like rebvio_hip_kf_hypothesis");
struct KfHypResult {
  KfPose pose;
  int inliers{0};
  int reserved{0};
};
static_assert(sizeof(KfHypResult) == sizeof(KfPose) + 8 && offsetof(KfHypResult, inliers) == sizeof(KfPose),
              "KfHypResult must stay layout-compatible with rebvio_hip_kf_hyp_result");
// One entry of a keyframe-window callback of rebvio::Rebvio: a keyframe (by the stamp of the map it was marked on), its pose relative
// to the record's map and the inliers of that alignment.
struct KfWindowPose {
  uint64_t kf_ts_us{0};
  KfPose pose;
  int inliers{0};
};

// Options of KeyframeSnapshot::fuseDepth, layout-compatible with the C-ABI's rebvio_hip_kf_fuse_opts (rebvio_hip.h defines every term).
// The defaults are rebvio_hip_default_kf_fuse_opts's; pixel_sigma <= 0 stands for the context's pixel_uncertainty and max_dist -1 for
// its search_range (fuseDepth fills them in).
struct KfFuseOpts {
  CloudFilter kf_filter;   // applied to the keyframe keylines
  double min_cos{0.9};     // the gradient test, where the snapshot has a non-zero normal; -1 disables it
  double pixel_sigma{0.0};
  double gate_sigma{3.0};  // innovation gate in standard deviations
  double q_abs{0.0};       // added in quadrature to sigma_rho before the update
  int max_dist{-1};        // 0..search_range cells between the projection and the keyline that owns its cell
  int reserved{0};
};
static_assert(sizeof(KfFuseOpts) == 56, "KfFuseOpts must stay layout-compatible with rebvio_hip_kf_fuse_opts");

// What KeyframeSnapshot::fuseDepth returns, layout-compatible with rebvio_hip_kf_fuse: associated = fused + gated + flat.
struct KfFuse {
  int candidates{0};  // the snapshot's size
  int associated{0};  // keylines that found an owner in the map's distance field
  int fused{0};       // ... and were updated
  int gated{0};       // ... failed the innovation gate or gave a non-finite update (left as they were)
  int flat{0};        // ... carried no information (left as they were)
  int clamped{0};     // among fused: rho ran into RHO_MIN or RHO_MAX
};
static_assert(sizeof(KfFuse) == 24, "KfFuse must stay layout-compatible with rebvio_hip_kf_fuse");

// Options of KeyframeSnapshot::handoverDepth, layout-compatible with the C-ABI's rebvio_hip_kf_handover_opts (rebvio_hip.h defines
// every term). The defaults are rebvio_hip_default_kf_handover_opts's; max_dist -1 stands for the context's search_range
// (handoverDepth fills it in).
struct KfHandoverOpts {
  CloudFilter kf_filter;   // applied to the outgoing keyframe's keylines
  double min_cos{0.9};     // the gradient test, where the outgoing snapshot has a non-zero normal; -1 disables it
  double gate_sigma{3.0};  // conflict gate in standard deviations
  double q_abs{0.0};       // added in quadrature to sigma_rho before it is propagated
  int max_dist{-1};        // 0..search_range cells between the projection and the keyline that owns its cell
  int reserved{0};
};
static_assert(sizeof(KfHandoverOpts) == 48, "KfHandoverOpts must stay layout-compatible with rebvio_hip_kf_handover_opts");

// What KeyframeSnapshot::handoverDepth returns, layout-compatible with rebvio_hip_kf_handover: claimed = adopted + kept + conflicts.
struct KfHandover {
  int candidates{0};    // the outgoing snapshot's size
  int associated{0};    // its keylines with an owner below the successor's size
  int out_of_range{0};  // ... whose propagated depth is not a usable one (they claim nothing)
  int claimed{0};       // successor slots with at least one claimant
  int adopted{0};       // ... that took the winner's depth
  int kept{0};          // ... that agreed with it and were no worse
  int conflicts{0};     // ... that disagreed with it beyond the gate
};
static_assert(sizeof(KfHandover) == 28, "KfHandover must stay layout-compatible with rebvio_hip_kf_handover");

// Edge chains and polylines of a map (EdgeMap::edgeChains / edgePolylines), layout-compatible with the C-ABI's rebvio_hip_chain_ref,
// rebvio_hip_polyline_opts and rebvio_hip_polyline; rebvio_hip.h defines succ / pred, head, rank, the chain table and a line exactly.
struct ChainRef {
  int head;    // a path's member without a predecessor; a cycle's smallest member index
  int rank;    // succ steps from head
  int length;  // members of the chain
  int flags;   // bit 0: the chain is cyclic
};
static_assert(sizeof(ChainRef) == 16, "ChainRef must stay layout-compatible with rebvio_hip_chain_ref");
struct PolylineOpts {
  CloudFilter filter;       // the cloud filter, applied per keyline
  int min_chain_length{8};  // >= 1: chains with fewer members give no line
  int reserved{0};
};
static_assert(sizeof(PolylineOpts) == 24, "PolylineOpts must stay layout-compatible with rebvio_hip_polyline_opts");
struct Polyline {
  int first_point;  // index of the line's first point in EdgePolylines::points
  int points;       // its number of points, consecutive along the edge
  int head;         // head of its chain
  int flags;        // bit 0: closed (the chain is cyclic and the line is all of it)
};
static_assert(sizeof(Polyline) == 16, "Polyline must stay layout-compatible with rebvio_hip_polyline");

// Straight segments of the polylines (EdgeMap::edgeSegments), layout-compatible with the C-ABI's rebvio_hip_segment_opts,
// rebvio_hip_line_segment and rebvio_hip_segment_counts; rebvio_hip.h defines the split rounds, a kept segment and the depth fit.
struct SegmentOpts {
  PolylineOpts poly;      // the polylines that are split
  float tol{1.0f};        // px: the largest deviation from its chord a segment keeps
  float min_length{4.0f}; // px between the end points of a kept segment
  int min_points{8};      // >= 2: points of a kept segment, both ends counted
  int max_rounds{16};     // 1..32 split rounds
};
static_assert(sizeof(SegmentOpts) == 40, "SegmentOpts must stay layout-compatible with rebvio_hip_segment_opts");
struct LineSegment {
  float xyz0[3], xyz1[3];  // the end points, posed as a cloud's points (zeros without a valid depth)
  float uv0[2], uv1[2];    // their pos_img
  float rho0, rho1, sigma_rho0, sigma_rho1;  // the fitted inverse depths at the ends and their standard deviations
  float max_dev2;          // px^2: the largest squared deviation of a member from the chord
  float chi2;              // the fit's weighted residual sum
  int first_point;         // index of the first end in EdgePolylines::points under the same options
  int points;              // members, both ends counted
  int line;                // index of its line
  int flags;               // bit 0: depth valid; bit 1: unresolved (max_rounds did not suffice)
};
static_assert(sizeof(LineSegment) == 80, "LineSegment must stay layout-compatible with rebvio_hip_line_segment");
struct SegmentCounts {
  int segments_all, kept, depth_valid, unresolved, rounds_used, points, lines, reserved;
};
static_assert(sizeof(SegmentCounts) == 32, "SegmentCounts must stay layout-compatible with rebvio_hip_segment_counts");

// What a point-cloud or keyframe-cloud callback of rebvio::Rebvio receives; `points` is valid during the callback only.
struct PointCloud {
  uint64_t ts_us;            // the odometry record's stamp (= the map's); keyframe cloud: the stamp of the record the keyframe was marked on
  CloudPose pose;            // R_global, Pos, K of that record: the points are metric, in the odometry's frame
  const CloudPoint* points;
  size_t size;
};

// What an edge-polyline callback of rebvio::Rebvio receives; the arrays are valid during the callback only.
struct EdgePolylines {
  uint64_t ts_us;            // the odometry record's stamp (= the map's)
  CloudPose pose;            // R_global, Pos, K of that record: the points are metric, in the odometry's frame
  const CloudPoint* points;  // in slot order: the points of a line are consecutive, ordered along the edge
  const int* refs;           // {head, rank} per point, two ints each
  size_t size;
  const Polyline* lines;
  size_t num_lines;
};

// What an edge-segment callback of rebvio::Rebvio receives; the array is valid during the callback only.
struct EdgeSegments {
  uint64_t ts_us;               // the odometry record's stamp (= the map's)
  CloudPose pose;               // R_global, Pos, K of that record: the end points are metric, in the odometry's frame
  const LineSegment* segments;  // the kept segments in point order
  size_t size;
  SegmentCounts counts;
};

}  // namespace types
}  // namespace rebvio
