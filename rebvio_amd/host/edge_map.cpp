#include "rebvio/edge_map.hpp"

#include <cstring>
#include <limits>

#include "session.hpp"

namespace rebvio {

using backend::check;

EdgeMap::EdgeMap(rebvio::Camera::SharedPtr camera, int size, uint64_t ts_us, rebvio::EdgeMapConfig::SharedPtr config)
    : config_(config), camera_(camera), ts_us_(ts_us), threshold_(-1.0) {
  keylines_.reserve(size);
}

EdgeMap::~EdgeMap() {
  if (handle_) rebvio_hip_map_release(handle_);
}

void EdgeMap::attach(rebvio_hip_ctx* ctx, rebvio_hip_map* handle, std::shared_ptr<void> keepalive) {
  keepalive_ = std::move(keepalive);
  ctx_ = ctx;
  handle_ = handle;
  invalidateMirror();
}

void EdgeMap::syncMirror() {
  if (mirror_valid_ || !handle_) return;
  const int n = rebvio_hip_map_size(handle_);
  if (n < 0) backend::fail("rebvio_hip_map_size", n);
  keylines_.resize((size_t)n);
  static_assert(sizeof(types::KeyLine) == sizeof(rebvio_hip_keyline), "AoS mirror layout");
  check("rebvio_hip_map_download",
        rebvio_hip_map_download(handle_, reinterpret_cast<rebvio_hip_keyline*>(keylines_.data()), nullptr));
  mirror_valid_ = true;
}

rebvio::types::KeyLine& EdgeMap::operator[](int idx) {
  syncMirror();
  return keylines_[idx];
}

int EdgeMap::size() {
  if (!handle_) return (int)keylines_.size();
  const int n = rebvio_hip_map_size(handle_);
  if (n < 0) backend::fail("rebvio_hip_map_size", n);
  return n;
}

std::vector<rebvio::types::KeyLine>& EdgeMap::keylines() {
  syncMirror();
  return keylines_;
}

uint64_t EdgeMap::ts_us() { return ts_us_; }

const types::Float& EdgeMap::threshold() const {
  if (handle_) threshold_ = rebvio_hip_map_threshold(handle_);
  return threshold_;
}

void EdgeMap::threshold(const types::Float& t) { threshold_ = t; }  // device maps take their threshold from detect()

rebvio::types::IntegratedImu& EdgeMap::imu() { return imu_; }

std::unordered_map<unsigned int, unsigned int>& EdgeMap::mask() {
  if (!mask_valid_ && handle_) {
    std::vector<int> dense((size_t)camera_->rows_ * camera_->cols_);
    check("rebvio_hip_map_download", rebvio_hip_map_download(handle_, nullptr, dense.data()));
    keylines_mask_.clear();
    for (size_t i = 0; i < dense.size(); ++i)
      if (dense[i] >= 0) keylines_mask_.emplace((unsigned)i, (unsigned)dense[i]);
    mask_valid_ = true;
  }
  return keylines_mask_;
}

types::Float EdgeMap::estimateQuantile(types::Float percentile, int num_bins) {
  float out = 1e3f;
  check("rebvio_hip_quantile", rebvio_hip_quantile(ctx_, handle_, percentile, num_bins, &out));
  return out;
}

void EdgeMap::rotateKeylines(const rebvio::types::Matrix3f& R) {
  float r[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r[i * 3 + j] = R(i, j);
  check("rebvio_hip_rotate", rebvio_hip_rotate(ctx_, handle_, r));
  invalidateMirror();
}

int EdgeMap::forwardMatch(rebvio::EdgeMap::SharedPtr map) {
  check("rebvio_hip_forward_match", rebvio_hip_forward_match(ctx_, handle_, map->handle_));
  map->invalidateMirror();
  return 0;  // the reference's count is order dependent and unused (rebvio.cpp:172)
}

int EdgeMap::searchMatch(const rebvio::types::KeyLine& keyline, const rebvio::types::Vector3f& vel, const rebvio::types::Matrix3f& Rvel,
                         const rebvio::types::Matrix3f& Rback, types::Float max_radius) {
  float v[3] = {vel[0], vel[1], vel[2]}, rv[9], rb[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      rv[i * 3 + j] = Rvel(i, j);
      rb[i * 3 + j] = Rback(i, j);
    }
  int idx = -1;
  check("rebvio_hip_search_match",
        rebvio_hip_search_match(ctx_, handle_, reinterpret_cast<const rebvio_hip_keyline*>(&keyline), v, rv, rb, max_radius, &idx));
  return idx;
}

int EdgeMap::directedMatch(rebvio::EdgeMap::SharedPtr map, const rebvio::types::Vector3f& vel, const rebvio::types::Matrix3f& Rvel,
                           const rebvio::types::Matrix3f& Rback, int& kf_matches, types::Float max_radius) {
  float v[3] = {vel[0], vel[1], vel[2]}, rv[9], rb[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      rv[i * 3 + j] = Rvel(i, j);
      rb[i * 3 + j] = Rback(i, j);
    }
  int n = 0, kf = 0;
  check("rebvio_hip_directed_match", rebvio_hip_directed_match(ctx_, handle_, map->handle_, v, rv, rb, max_radius, &n, &kf));
  kf_matches = kf;
  invalidateMirror();
  return n;
}

int EdgeMap::regularize1Iter() {
  int n = 0;
  check("rebvio_hip_regularize", rebvio_hip_regularize(ctx_, handle_, &n));
  invalidateMirror();
  return n;
}

std::vector<rebvio::types::CloudPoint> EdgeMap::pointCloud(const rebvio::types::CloudFilter& filter, const rebvio::types::CloudPose& pose) {
  static_assert(sizeof(types::CloudPoint) == sizeof(rebvio_hip_cloud_point) && sizeof(types::CloudFilter) == sizeof(rebvio_hip_cloud_filter) &&
                    sizeof(types::CloudPose) == sizeof(rebvio_hip_cloud_pose), "point-cloud types mirror the C-ABI's");
  std::vector<rebvio::types::CloudPoint> points((size_t)size());
  int count = 0;
  check("rebvio_hip_map_point_cloud",
        rebvio_hip_map_point_cloud(handle_, reinterpret_cast<const rebvio_hip_cloud_filter*>(&filter),
                                   reinterpret_cast<const rebvio_hip_cloud_pose*>(&pose),
                                   reinterpret_cast<rebvio_hip_cloud_point*>(points.data()), (int)points.size(), &count));
  points.resize((size_t)count);
  return points;
}

rebvio::types::DepthPriorCounts EdgeMap::fuseDepthImage(const rebvio::types::DepthImage& image, const rebvio::types::DepthPriorOpts& opts,
                                                        std::vector<int>* outcome) {
  static_assert(sizeof(types::DepthPriorOpts) == sizeof(rebvio_hip_depth_prior_opts) &&
                    offsetof(types::DepthPriorOpts, unit) == offsetof(rebvio_hip_depth_prior_opts, unit) &&
                    offsetof(types::DepthPriorOpts, reserved) == offsetof(rebvio_hip_depth_prior_opts, reserved) &&
                    sizeof(types::DepthPriorCounts) == sizeof(rebvio_hip_depth_prior_counts) &&
                    offsetof(types::DepthPriorCounts, clamped) == offsetof(rebvio_hip_depth_prior_counts, clamped) &&
                    (int)types::DEPTH_U16 == REBVIO_HIP_DEPTH_U16 && (int)types::DEPTH_F32 == REBVIO_HIP_DEPTH_F32,
                "depth-prior types mirror the C-ABI's");
  if (image.rows != (int)camera_->rows_ || image.cols != (int)camera_->cols_)
    backend::fail("EdgeMap::fuseDepthImage: the depth image does not have the camera's size", -3);
  types::DepthPriorOpts o = opts;
  if (image.unit > 0.0) o.unit = image.unit;
  if (outcome) outcome->assign((size_t)size(), 0);
  types::DepthPriorCounts counts;
  check("rebvio_hip_map_fuse_depth_image",
        rebvio_hip_map_fuse_depth_image(handle_, image.data, image.pitch, image.format, reinterpret_cast<const rebvio_hip_depth_prior_opts*>(&o),
                                        reinterpret_cast<rebvio_hip_depth_prior_counts*>(&counts), outcome && !outcome->empty() ? outcome->data() : nullptr));
  invalidateMirror();
  return counts;
}

rebvio::types::StereoPriorCounts EdgeMap::fuseStereo(const EdgeMap& right, const rebvio::types::StereoPriorOpts& opts, std::vector<int>* outcome,
                                                     std::vector<int>* winner) {
  static_assert(sizeof(types::StereoPriorOpts) == sizeof(rebvio_hip_stereo_prior_opts) &&
                    offsetof(types::StereoPriorOpts, row_tol) == offsetof(rebvio_hip_stereo_prior_opts, row_tol) &&
                    offsetof(types::StereoPriorOpts, sigma_px) == offsetof(rebvio_hip_stereo_prior_opts, sigma_px) &&
                    offsetof(types::StereoPriorOpts, q_abs) == offsetof(rebvio_hip_stereo_prior_opts, q_abs) &&
                    offsetof(types::StereoPriorOpts, reserved) == offsetof(rebvio_hip_stereo_prior_opts, reserved) &&
                    sizeof(types::StereoPriorCounts) == sizeof(rebvio_hip_stereo_prior_counts) &&
                    offsetof(types::StereoPriorCounts, clamped) == offsetof(rebvio_hip_stereo_prior_counts, clamped),
                "stereo-prior types mirror the C-ABI's");
  if (outcome) outcome->assign((size_t)size(), 0);
  if (winner) winner->assign((size_t)size(), -1);
  types::StereoPriorCounts counts;
  check("rebvio_hip_map_fuse_stereo",
        rebvio_hip_map_fuse_stereo(handle_, right.handle_, reinterpret_cast<const rebvio_hip_stereo_prior_opts*>(&opts),
                                   reinterpret_cast<rebvio_hip_stereo_prior_counts*>(&counts), outcome && !outcome->empty() ? outcome->data() : nullptr,
                                   winner && !winner->empty() ? winner->data() : nullptr));
  invalidateMirror();
  return counts;
}

EdgeMap::EdgeChains EdgeMap::edgeChains() {
  static_assert(sizeof(types::ChainRef) == sizeof(rebvio_hip_chain_ref) && offsetof(types::ChainRef, flags) == offsetof(rebvio_hip_chain_ref, flags),
                "chain records mirror the C-ABI's");
  EdgeChains out;
  const size_t n = (size_t)size();
  out.refs.resize(n);
  out.order.resize(n);
  out.starts.resize(n + 1);
  int nk = 0, nc = 0;
  check("rebvio_hip_map_edge_chains",
        rebvio_hip_map_edge_chains(handle_, reinterpret_cast<rebvio_hip_chain_ref*>(out.refs.data()), (int)n, out.order.data(), out.starts.data(),
                                   (int)n + 1, &nk, &nc));
  out.refs.resize((size_t)nk);  // (nk = the map's size)
  out.order.resize((size_t)nk);
  out.starts.resize((size_t)nc + 1);
  return out;
}

EdgeMap::EdgePolylines EdgeMap::edgePolylines(const rebvio::types::PolylineOpts& opts, const rebvio::types::CloudPose& pose) {
  static_assert(sizeof(types::PolylineOpts) == sizeof(rebvio_hip_polyline_opts) && sizeof(types::Polyline) == sizeof(rebvio_hip_polyline) &&
                    offsetof(types::PolylineOpts, min_chain_length) == offsetof(rebvio_hip_polyline_opts, min_chain_length) &&
                    offsetof(types::Polyline, head) == offsetof(rebvio_hip_polyline, head), "polyline types mirror the C-ABI's");
  EdgePolylines out;
  const size_t n = (size_t)size();
  out.points.resize(n);
  out.refs.resize(n);
  out.lines.resize(n);
  int np = 0, nl = 0;
  check("rebvio_hip_map_edge_polylines",
        rebvio_hip_map_edge_polylines(handle_, reinterpret_cast<const rebvio_hip_polyline_opts*>(&opts),
                                      reinterpret_cast<const rebvio_hip_cloud_pose*>(&pose), reinterpret_cast<rebvio_hip_cloud_point*>(out.points.data()),
                                      reinterpret_cast<int*>(out.refs.data()), (int)n, reinterpret_cast<rebvio_hip_polyline*>(out.lines.data()), (int)n,
                                      &np, &nl));
  out.points.resize((size_t)np);  // (np, nl <= the map's size: nothing was cut)
  out.refs.resize((size_t)np);
  out.lines.resize((size_t)nl);
  return out;
}

EdgeMap::EdgeSegments EdgeMap::edgeSegments(const rebvio::types::SegmentOpts& opts, const rebvio::types::CloudPose& pose) {
  static_assert(sizeof(types::SegmentOpts) == sizeof(rebvio_hip_segment_opts) && sizeof(types::LineSegment) == sizeof(rebvio_hip_line_segment) &&
                    sizeof(types::SegmentCounts) == sizeof(rebvio_hip_segment_counts) &&
                    offsetof(types::SegmentOpts, max_rounds) == offsetof(rebvio_hip_segment_opts, max_rounds) &&
                    offsetof(types::LineSegment, rho0) == offsetof(rebvio_hip_line_segment, rho0) &&
                    offsetof(types::LineSegment, flags) == offsetof(rebvio_hip_line_segment, flags) &&
                    offsetof(types::SegmentCounts, lines) == offsetof(rebvio_hip_segment_counts, lines), "segment types mirror the C-ABI's");
  EdgeSegments out;
  const size_t n = (size_t)size();
  out.segments.resize(n);  // (a map of n keylines has fewer than n segments: nothing is cut)
  check("rebvio_hip_map_edge_segments",
        rebvio_hip_map_edge_segments(handle_, reinterpret_cast<const rebvio_hip_segment_opts*>(&opts),
                                     reinterpret_cast<const rebvio_hip_cloud_pose*>(&pose),
                                     reinterpret_cast<rebvio_hip_line_segment*>(out.segments.data()), (int)n,
                                     reinterpret_cast<rebvio_hip_segment_counts*>(&out.counts)));
  out.segments.resize((size_t)out.counts.kept);
  return out;
}

void EdgeMap::markKeyframe() {
  check("rebvio_hip_map_mark_keyframe", rebvio_hip_map_mark_keyframe(ctx_, handle_));
  invalidateMirror();
}

std::vector<rebvio::types::KfMatch> EdgeMap::keyframeMatches(int kf_size) {
  static_assert(sizeof(types::KfMatch) == sizeof(rebvio_hip_kf_match), "keyframe correspondences mirror the C-ABI's");
  std::vector<rebvio::types::KfMatch> out((size_t)(kf_size > 0 ? kf_size : 0));
  int count = 0;
  check("rebvio_hip_map_keyframe_matches",
        rebvio_hip_map_keyframe_matches(handle_, kf_size, reinterpret_cast<rebvio_hip_kf_match*>(out.data()), (int)out.size(), &count));
  out.resize((size_t)count);  // (count <= kf_size: one record per keyframe keyline at most)
  return out;
}

void KeyframeSnapshot::reset() {
  if (handle_) rebvio_hip_kf_snapshot_release(handle_);
  handle_ = nullptr;
  keepalive_.reset();
}

// ---- place recognition ----------------------------------------------------------------------------------------------------------
static_assert(sizeof(types::PlaceMatch) == sizeof(rebvio_hip_place_match) && offsetof(types::PlaceMatch, distance) == offsetof(rebvio_hip_place_match, distance) &&
                  offsetof(types::PlaceMatch, index) == offsetof(rebvio_hip_place_match, index) &&
                  offsetof(types::PlaceMatch, tag) == offsetof(rebvio_hip_place_match, tag) && types::kPlaceWords == REBVIO_HIP_PLACE_WORDS &&
                  types::kPlaceTopKMax == REBVIO_HIP_PLACE_TOPK_MAX,
              "place records mirror the C-ABI's");

rebvio::types::PlaceSignature EdgeMap::placeSignature(int* counted) const {
  types::PlaceSignature sig{};
  int n = 0;
  check("rebvio_hip_map_place_signature", rebvio_hip_map_place_signature(handle_, sig.data(), &n));
  if (counted) *counted = n;
  return sig;
}

rebvio::PlaceDb EdgeMap::placeDb(int capacity) const {
  rebvio_hip_place_db* h = nullptr;
  check("rebvio_hip_place_db_create", rebvio_hip_place_db_create(ctx_, capacity, &h));
  return rebvio::PlaceDb(h, capacity, keepalive_);
}

void PlaceDb::reset() {
  if (handle_) rebvio_hip_place_db_release(handle_);
  handle_ = nullptr;
  keepalive_.reset();
}

int PlaceDb::size() const {
  const int n = rebvio_hip_place_db_size(handle_);
  if (n < 0) check("rebvio_hip_place_db_size", n);
  return n;
}

void PlaceDb::clear() { check("rebvio_hip_place_db_clear", rebvio_hip_place_db_clear(handle_)); }

int PlaceDb::add(const rebvio::EdgeMap& map, uint64_t tag) {
  if (handle_ && size() >= capacity_) return -1;
  int index = -1;
  check("rebvio_hip_place_db_add", rebvio_hip_place_db_add(handle_, map.handle(), tag, &index));
  return index;
}

int PlaceDb::addSignature(const rebvio::types::PlaceSignature& signature, int counted, uint64_t tag) {
  if (handle_ && size() >= capacity_) return -1;
  int index = -1;
  check("rebvio_hip_place_db_add_signature", rebvio_hip_place_db_add_signature(handle_, signature.data(), counted, tag, &index));
  return index;
}

rebvio::types::PlaceSignature PlaceDb::entry(int index, int* counted, uint64_t* tag) const {
  types::PlaceSignature sig{};
  check("rebvio_hip_place_db_entry", rebvio_hip_place_db_entry(handle_, index, sig.data(), counted, tag));
  return sig;
}

std::vector<rebvio::types::PlaceMatch> PlaceDb::query(const rebvio::EdgeMap& map, int k, int exclude_last) const {
  std::vector<types::PlaceMatch> out((size_t)(k > 0 && k <= types::kPlaceTopKMax ? k : 0));
  int n = 0;
  check("rebvio_hip_place_db_query",
        rebvio_hip_place_db_query(handle_, map.handle(), k, exclude_last, reinterpret_cast<rebvio_hip_place_match*>(out.data()), &n));
  out.resize((size_t)n);
  return out;
}

std::vector<rebvio::types::PlaceMatch> PlaceDb::querySignature(const rebvio::types::PlaceSignature& signature, int k, int exclude_last) const {
  std::vector<types::PlaceMatch> out((size_t)(k > 0 && k <= types::kPlaceTopKMax ? k : 0));
  int n = 0;
  check("rebvio_hip_place_db_query_signature",
        rebvio_hip_place_db_query_signature(handle_, signature.data(), k, exclude_last, reinterpret_cast<rebvio_hip_place_match*>(out.data()), &n));
  out.resize((size_t)n);
  return out;
}

rebvio::KeyframeSnapshot EdgeMap::keyframeSnapshot() {
  rebvio_hip_kf_snapshot* h = nullptr;
  const int rc = rebvio_hip_map_keyframe_snapshot(ctx_, handle_, &h);
  rebvio::KeyframeSnapshot snap(h, keepalive_);  // (a handle that came with an error is still the caller's to release)
  check("rebvio_hip_map_keyframe_snapshot", rc);
  return snap;
}

rebvio::types::KfPose EdgeMap::keyframePose(const rebvio::KeyframeSnapshot& snapshot, const rebvio::types::KfPoseOpts& opts,
                                            const rebvio::types::KfPose* guess) {
  static_assert(sizeof(types::KfPose) == sizeof(rebvio_hip_kf_pose) && sizeof(types::KfPoseOpts) == sizeof(rebvio_hip_kf_pose_opts) &&
                    offsetof(types::KfPose, status) == offsetof(rebvio_hip_kf_pose, status) &&
                    offsetof(types::KfPose, cost) == offsetof(rebvio_hip_kf_pose, cost) &&
                    offsetof(types::KfPoseOpts, min_used) == offsetof(rebvio_hip_kf_pose_opts, min_used),
                "keyframe pose types mirror the C-ABI's");
  rebvio::types::KfPose out;
  check("rebvio_hip_map_keyframe_pose",
        rebvio_hip_map_keyframe_pose(handle_, snapshot.handle(), reinterpret_cast<const rebvio_hip_kf_pose_opts*>(&opts),
                                     guess ? guess->R : nullptr, guess ? guess->t : nullptr, reinterpret_cast<rebvio_hip_kf_pose*>(&out)));
  return out;
}

void KeyframeSnapshot::addNormals(const rebvio::EdgeMap& map) {
  check("rebvio_hip_kf_snapshot_add_normals", rebvio_hip_kf_snapshot_add_normals(handle_, map.handle()));
}

std::vector<rebvio::types::CloudPoint> KeyframeSnapshot::pointCloud(const rebvio::types::CloudFilter& filter,
                                                                    const rebvio::types::CloudPose& pose) const {
  const rebvio_hip_cloud_filter* f = reinterpret_cast<const rebvio_hip_cloud_filter*>(&filter);
  const rebvio_hip_cloud_pose* p = reinterpret_cast<const rebvio_hip_cloud_pose*>(&pose);
  int count = 0;  // the count first: a snapshot's size lives on the device
  check("rebvio_hip_kf_snapshot_point_cloud", rebvio_hip_kf_snapshot_point_cloud(handle_, f, p, nullptr, 0, &count));
  std::vector<rebvio::types::CloudPoint> points((size_t)count);
  if (count > 0)
    check("rebvio_hip_kf_snapshot_point_cloud",
          rebvio_hip_kf_snapshot_point_cloud(handle_, f, p, reinterpret_cast<rebvio_hip_cloud_point*>(points.data()), count, &count));
  points.resize((size_t)count);
  return points;
}

rebvio::types::KfFuse KeyframeSnapshot::fuseDepth(const rebvio::EdgeMap& map, const rebvio::types::KfPose& pose,
                                                  const rebvio::types::KfFuseOpts& opts, std::vector<int>* assoc) {
  static_assert(sizeof(types::KfFuseOpts) == sizeof(rebvio_hip_kf_fuse_opts) &&
                    offsetof(types::KfFuseOpts, min_cos) == offsetof(rebvio_hip_kf_fuse_opts, min_cos) &&
                    offsetof(types::KfFuseOpts, pixel_sigma) == offsetof(rebvio_hip_kf_fuse_opts, pixel_sigma) &&
                    offsetof(types::KfFuseOpts, gate_sigma) == offsetof(rebvio_hip_kf_fuse_opts, gate_sigma) &&
                    offsetof(types::KfFuseOpts, q_abs) == offsetof(rebvio_hip_kf_fuse_opts, q_abs) &&
                    offsetof(types::KfFuseOpts, max_dist) == offsetof(rebvio_hip_kf_fuse_opts, max_dist) &&
                    offsetof(types::KfFuseOpts, reserved) == offsetof(rebvio_hip_kf_fuse_opts, reserved),
                "depth fusion options mirror the C-ABI's");
  static_assert(sizeof(types::KfFuse) == sizeof(rebvio_hip_kf_fuse) && offsetof(types::KfFuse, associated) == offsetof(rebvio_hip_kf_fuse, associated) &&
                    offsetof(types::KfFuse, fused) == offsetof(rebvio_hip_kf_fuse, fused) && offsetof(types::KfFuse, gated) == offsetof(rebvio_hip_kf_fuse, gated) &&
                    offsetof(types::KfFuse, flat) == offsetof(rebvio_hip_kf_fuse, flat) && offsetof(types::KfFuse, clamped) == offsetof(rebvio_hip_kf_fuse, clamped),
                "depth fusion counts mirror the C-ABI's");
  rebvio_hip_kf_fuse_opts o;
  std::memcpy(&o, &opts, sizeof(o));
  if (!(o.pixel_sigma > 0.0) || o.max_dist < 0) {  // the context's pixel_uncertainty / search_range
    rebvio_hip_kf_fuse_opts def;
    rebvio_hip_default_kf_fuse_opts(map.ctx(), &def);
    if (!(o.pixel_sigma > 0.0)) o.pixel_sigma = def.pixel_sigma;
    if (o.max_dist < 0) o.max_dist = def.max_dist;
  }
  if (assoc) {
    int n = 0;
    check("rebvio_hip_kf_snapshot_download", handle_ ? rebvio_hip_kf_snapshot_download(handle_, nullptr, nullptr, 0, &n) : 0);
    assoc->assign((size_t)n, std::numeric_limits<int>::min());
  }
  rebvio::types::KfFuse out;
  check("rebvio_hip_kf_snapshot_fuse_depth",
        rebvio_hip_kf_snapshot_fuse_depth(handle_, map.handle(), &o, pose.R, pose.t, reinterpret_cast<rebvio_hip_kf_fuse*>(&out),
                                          assoc && !assoc->empty() ? assoc->data() : nullptr));
  return out;
}

rebvio::types::KfHandover KeyframeSnapshot::handoverDepth(const rebvio::KeyframeSnapshot& src, const rebvio::EdgeMap& map,
                                                          const rebvio::types::KfPose& pose, const rebvio::types::KfHandoverOpts& opts,
                                                          std::vector<int>* assoc) {
  static_assert(sizeof(types::KfHandoverOpts) == sizeof(rebvio_hip_kf_handover_opts) &&
                    offsetof(types::KfHandoverOpts, min_cos) == offsetof(rebvio_hip_kf_handover_opts, min_cos) &&
                    offsetof(types::KfHandoverOpts, gate_sigma) == offsetof(rebvio_hip_kf_handover_opts, gate_sigma) &&
                    offsetof(types::KfHandoverOpts, q_abs) == offsetof(rebvio_hip_kf_handover_opts, q_abs) &&
                    offsetof(types::KfHandoverOpts, max_dist) == offsetof(rebvio_hip_kf_handover_opts, max_dist) &&
                    offsetof(types::KfHandoverOpts, reserved) == offsetof(rebvio_hip_kf_handover_opts, reserved),
                "depth hand-over options mirror the C-ABI's");
  static_assert(sizeof(types::KfHandover) == sizeof(rebvio_hip_kf_handover) &&
                    offsetof(types::KfHandover, associated) == offsetof(rebvio_hip_kf_handover, associated) &&
                    offsetof(types::KfHandover, out_of_range) == offsetof(rebvio_hip_kf_handover, out_of_range) &&
                    offsetof(types::KfHandover, claimed) == offsetof(rebvio_hip_kf_handover, claimed) &&
                    offsetof(types::KfHandover, adopted) == offsetof(rebvio_hip_kf_handover, adopted) &&
                    offsetof(types::KfHandover, kept) == offsetof(rebvio_hip_kf_handover, kept) &&
                    offsetof(types::KfHandover, conflicts) == offsetof(rebvio_hip_kf_handover, conflicts),
                "depth hand-over counts mirror the C-ABI's");
  rebvio_hip_kf_handover_opts o;
  std::memcpy(&o, &opts, sizeof(o));
  if (o.max_dist < 0) {  // the context's search_range
    rebvio_hip_kf_handover_opts def;
    rebvio_hip_default_kf_handover_opts(map.ctx(), &def);
    o.max_dist = def.max_dist;
  }
  if (assoc) {
    int n = 0;
    check("rebvio_hip_kf_snapshot_download", src.handle() ? rebvio_hip_kf_snapshot_download(src.handle(), nullptr, nullptr, 0, &n) : 0);
    assoc->assign((size_t)n, std::numeric_limits<int>::min());
  }
  rebvio::types::KfHandover out;
  check("rebvio_hip_kf_snapshot_handover_depth",
        rebvio_hip_kf_snapshot_handover_depth(handle_, src.handle(), map.handle(), &o, pose.R, pose.t,
                                              reinterpret_cast<rebvio_hip_kf_handover*>(&out),
                                              assoc && !assoc->empty() ? assoc->data() : nullptr));
  return out;
}

rebvio::types::KfPose EdgeMap::keyframeAlign(const rebvio::KeyframeSnapshot& snapshot, const rebvio::types::KfAlignOpts& opts,
                                             const rebvio::types::KfPose* guess, std::vector<int>* assoc) {
  static_assert(sizeof(types::KfAlignOpts) == sizeof(rebvio_hip_kf_align_opts) &&
                    offsetof(types::KfAlignOpts, huber_px) == offsetof(rebvio_hip_kf_align_opts, huber_px) &&
                    offsetof(types::KfAlignOpts, min_cos) == offsetof(rebvio_hip_kf_align_opts, min_cos) &&
                    offsetof(types::KfAlignOpts, max_dist) == offsetof(rebvio_hip_kf_align_opts, max_dist) &&
                    offsetof(types::KfAlignOpts, max_iter) == offsetof(rebvio_hip_kf_align_opts, max_iter) &&
                    offsetof(types::KfAlignOpts, min_used) == offsetof(rebvio_hip_kf_align_opts, min_used),
                "keyframe alignment options mirror the C-ABI's");
  rebvio_hip_kf_align_opts o;
  std::memcpy(&o, &opts, sizeof(o));
  if (o.max_dist < 0) {  // the context's search_range
    rebvio_hip_kf_align_opts def;
    rebvio_hip_default_kf_align_opts(ctx_, &def);
    o.max_dist = def.max_dist;
  }
  if (assoc) {
    int n = 0;
    check("rebvio_hip_kf_snapshot_download", snapshot.handle() ? rebvio_hip_kf_snapshot_download(snapshot.handle(), nullptr, nullptr, 0, &n) : 0);
    assoc->assign((size_t)n, -1);
  }
  rebvio::types::KfPose out;
  check("rebvio_hip_map_keyframe_align",
        rebvio_hip_map_keyframe_align(handle_, snapshot.handle(), &o, guess ? guess->R : nullptr, guess ? guess->t : nullptr,
                                      reinterpret_cast<rebvio_hip_kf_pose*>(&out), assoc && !assoc->empty() ? assoc->data() : nullptr));
  return out;
}

std::vector<rebvio::types::KfHypResult> EdgeMap::keyframeAlignMany(const std::vector<rebvio::types::KfHypothesis>& hypotheses,
                                                                   const rebvio::types::KfAlignOpts& opts) {
  static_assert(sizeof(types::KfHypResult) == sizeof(rebvio_hip_kf_hyp_result) &&
                    offsetof(types::KfHypResult, inliers) == offsetof(rebvio_hip_kf_hyp_result, inliers) &&
                    sizeof(types::KfHypothesis) == sizeof(rebvio_hip_kf_hypothesis) &&
                    offsetof(types::KfHypothesis, R0) == offsetof(rebvio_hip_kf_hypothesis, R0) &&
                    offsetof(types::KfHypothesis, t0) == offsetof(rebvio_hip_kf_hypothesis, t0),
                "batched alignment types mirror the C-ABI's");
  rebvio_hip_kf_align_opts o;
  std::memcpy(&o, &opts, sizeof(o));
  if (o.max_dist < 0) {  // the context's search_range
    rebvio_hip_kf_align_opts def;
    rebvio_hip_default_kf_align_opts(ctx_, &def);
    o.max_dist = def.max_dist;
  }
  std::vector<rebvio_hip_kf_hypothesis> hyp(hypotheses.size());
  for (size_t h = 0; h < hyp.size(); ++h) {
    hyp[h].snap = hypotheses[h].snapshot ? hypotheses[h].snapshot->handle() : nullptr;
    std::memcpy(hyp[h].R0, hypotheses[h].R0, sizeof(hyp[h].R0));
    std::memcpy(hyp[h].t0, hypotheses[h].t0, sizeof(hyp[h].t0));
  }
  std::vector<rebvio::types::KfHypResult> out(hyp.size());
  check("rebvio_hip_map_keyframe_align_many",
        rebvio_hip_map_keyframe_align_many(handle_, hyp.empty() ? nullptr : hyp.data(), (int)hyp.size(), &o,
                                           reinterpret_cast<rebvio_hip_kf_hyp_result*>(out.data())));
  return out;
}

int keyframeAlignBest(const std::vector<rebvio::types::KfHypResult>& results, int min_inliers) {
  const int rc = rebvio_hip_kf_align_best(reinterpret_cast<const rebvio_hip_kf_hyp_result*>(results.data()), (int)results.size(), min_inliers);
  if (rc < -1) check("rebvio_hip_kf_align_best", rc);
  return rc;
}

std::vector<rebvio::types::KfHypothesis> keyframeHypothesesAround(const rebvio::KeyframeSnapshot& snapshot, const double R[9], const double t[3],
                                                                  double rot_step, double trans_step) {
  rebvio_hip_kf_hypothesis h13[13];
  check("rebvio_hip_kf_hypotheses_around", rebvio_hip_kf_hypotheses_around(snapshot.handle(), R, t, rot_step, trans_step, h13));
  std::vector<rebvio::types::KfHypothesis> out(13);
  for (int k = 0; k < 13; ++k) {
    out[k].snapshot = &snapshot;
    std::memcpy(out[k].R0, h13[k].R0, sizeof(h13[k].R0));
    std::memcpy(out[k].t0, h13[k].t0, sizeof(h13[k].t0));
  }
  return out;
}

}  // namespace rebvio
