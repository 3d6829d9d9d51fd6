// rebvio::EdgeMap — per-frame keyline container + the per-keyline tracking operations (reference edge_map.hpp:28-135).
// Here the keylines live on the GPU (SoA, owned by a pooled rebvio_hip_map); the host-visible std::vector<KeyLine>,
// operator[] and mask() are lazily downloaded mirrors, so callers such as ros_rebvio.cpp:44-46 keep working and
// nobody pays a device->host copy unless they look.
#pragma once

#include <array>
#include <memory>
#include <unordered_map>
#include <vector>

#include "rebvio/types/imu.hpp"
#include "rebvio/types/keyline.hpp"
#include "rebvio/types/depth_image.hpp"
#include "rebvio/types/point_cloud.hpp"
#include "rebvio/types/place.hpp"
#include "rebvio/types/stereo_prior.hpp"

struct rebvio_hip_map;
struct rebvio_hip_ctx;
struct rebvio_hip_kf_snapshot;
struct rebvio_hip_place_db;

namespace rebvio {

class EdgeMap;

// A keyframe as it was when the snapshot was taken (EdgeMap::keyframeSnapshot): owns the backend's handle and releases it; the
// handle's device memory goes with its context at the latest. Move-only.
class KeyframeSnapshot {
 public:
  KeyframeSnapshot() = default;
  KeyframeSnapshot(rebvio_hip_kf_snapshot* handle, std::shared_ptr<void> keepalive) : keepalive_(std::move(keepalive)), handle_(handle) {}
  ~KeyframeSnapshot() { reset(); }
  KeyframeSnapshot(KeyframeSnapshot&& o) noexcept : keepalive_(std::move(o.keepalive_)), handle_(o.handle_) { o.handle_ = nullptr; }
  KeyframeSnapshot& operator=(KeyframeSnapshot&& o) noexcept {
    if (this != &o) {
      reset();
      keepalive_ = std::move(o.keepalive_);
      handle_ = o.handle_;
      o.handle_ = nullptr;
    }
    return *this;
  }
  KeyframeSnapshot(const KeyframeSnapshot&) = delete;
  KeyframeSnapshot& operator=(const KeyframeSnapshot&) = delete;
  void reset();
  // keeps gradient / gradient_norm of `map`'s keylines next to the snapshot, for the gradient test of EdgeMap::keyframeAlign
  // (rebvio_hip_kf_snapshot_add_normals; queued on the track stream). `map` is the map the snapshot was taken from, where it was taken.
  void addNormals(const rebvio::EdgeMap& map);
  // folds `map`, seen from `pose` (X_cur = R X_kf + t, e.g. what EdgeMap::keyframeAlign returned for it), into this snapshot's rho /
  // sigma_rho: one scalar Kalman update per keyline that finds an owner in map's distance field (rebvio_hip_kf_snapshot_fuse_depth;
  // synchronous, from the tracking thread). assoc: per keyframe keyline the owner i when fused, -1 - i when gated or flat, INT_MIN
  // when not associated. Fusing one map twice counts its pixels twice.
  rebvio::types::KfFuse fuseDepth(const rebvio::EdgeMap& map, const rebvio::types::KfPose& pose,
                                  const rebvio::types::KfFuseOpts& opts = rebvio::types::KfFuseOpts(), std::vector<int>* assoc = nullptr);
  // takes over the refined depths of `src`, the outgoing keyframe's snapshot, where they are better than this snapshot's own
  // (rebvio_hip_kf_snapshot_handover_depth; synchronous, from the tracking thread). This snapshot must have been taken from `map`;
  // `pose` is X_cur = R X_kf + t of src against map (e.g. what EdgeMap::keyframeAlign returned for it). src is only read; the two
  // estimates of a slot are never combined. assoc: per src keyline the slot i when it won an adopted slot, -1 - i for any other
  // associated keyline, INT_MIN when not associated.
  rebvio::types::KfHandover handoverDepth(const rebvio::KeyframeSnapshot& src, const rebvio::EdgeMap& map, const rebvio::types::KfPose& pose,
                                          const rebvio::types::KfHandoverOpts& opts = rebvio::types::KfHandoverOpts(),
                                          std::vector<int>* assoc = nullptr);
  // the snapshot's depth-bearing keylines - as marked, or as fuseDepth has refined them - as a point cloud, filtered and posed on
  // the device (rebvio_hip_kf_snapshot_point_cloud says exactly which keylines and where; synchronous, from the tracking thread).
  // The default pose is the keyframe's own frame in keyframe depth units; `keyline` is the index in the snapshot and
  // gradient_norm is 0: a snapshot does not keep it.
  std::vector<rebvio::types::CloudPoint> pointCloud(const rebvio::types::CloudFilter& filter = rebvio::types::CloudFilter(),
                                                    const rebvio::types::CloudPose& pose = rebvio::types::CloudPose()) const;
  explicit operator bool() const { return handle_ != nullptr; }
  rebvio_hip_kf_snapshot* handle() const { return handle_; }

 private:
  std::shared_ptr<void> keepalive_;  // the backend context the handle belongs to (as EdgeMap's)
  rebvio_hip_kf_snapshot* handle_ = nullptr;
};

// A device-resident database of place signatures (EdgeMap::placeDb; rebvio_hip.h "Place recognition"): add() the maps keyframes are
// marked on, query() with a later map - the entries whose edges look like it, nearest first, are the keyframes to hand to
// EdgeMap::keyframeAlignMany. Owns the backend's handle and releases it; the device memory goes with its context at the latest.
// Move-only. Every call runs on the context's track stream, from the tracking thread; the maps are of the database's context.
class PlaceDb {
 public:
  PlaceDb() = default;
  PlaceDb(rebvio_hip_place_db* handle, int capacity, std::shared_ptr<void> keepalive)
      : keepalive_(std::move(keepalive)), handle_(handle), capacity_(capacity) {}
  ~PlaceDb() { reset(); }
  PlaceDb(PlaceDb&& o) noexcept : keepalive_(std::move(o.keepalive_)), handle_(o.handle_), capacity_(o.capacity_) { o.handle_ = nullptr; }
  PlaceDb& operator=(PlaceDb&& o) noexcept {
    if (this != &o) {
      reset();
      keepalive_ = std::move(o.keepalive_);
      handle_ = o.handle_;
      capacity_ = o.capacity_;
      o.handle_ = nullptr;
    }
    return *this;
  }
  PlaceDb(const PlaceDb&) = delete;
  PlaceDb& operator=(const PlaceDb&) = delete;
  void reset();
  int size() const;
  int capacity() const { return capacity_; }
  void clear();
  // the signature of `map` as the next entry (queued, no host wait) -> its index, or -1 when the database is full
  int add(const rebvio::EdgeMap& map, uint64_t tag);
  // a saved entry back in (synchronous) -> its index, or -1 when the database is full
  int addSignature(const rebvio::types::PlaceSignature& signature, int counted, uint64_t tag);
  // one entry (synchronous; after a queued add it waits for it). counted, tag: null, or where they go
  rebvio::types::PlaceSignature entry(int index, int* counted = nullptr, uint64_t* tag = nullptr) const;
  // the k <= 16 entries nearest to the map's signature among all but the last exclude_last, ascending (distance, index); synchronous
  std::vector<rebvio::types::PlaceMatch> query(const rebvio::EdgeMap& map, int k, int exclude_last = 0) const;
  std::vector<rebvio::types::PlaceMatch> querySignature(const rebvio::types::PlaceSignature& signature, int k, int exclude_last = 0) const;
  explicit operator bool() const { return handle_ != nullptr; }
  rebvio_hip_place_db* handle() const { return handle_; }

 private:
  std::shared_ptr<void> keepalive_;  // the backend context the handle belongs to (as EdgeMap's)
  rebvio_hip_place_db* handle_ = nullptr;
  int capacity_ = 0;
};

// the best of keyframeAlignMany's results (rebvio_hip_kf_align_best): status 0 and inliers >= min_inliers; the most inliers, then the
// smaller cost, then the lower index; -1 when none qualifies
int keyframeAlignBest(const std::vector<rebvio::types::KfHypResult>& results, int min_inliers = 0);
// 13 starts around the guess (R, t) for `snapshot` (rebvio_hip_kf_hypotheses_around): the guess, +- rot_step about x, y, z,
// +- trans_step along x, y, z
std::vector<rebvio::types::KfHypothesis> keyframeHypothesesAround(const rebvio::KeyframeSnapshot& snapshot, const double R[9], const double t[3],
                                                                  double rot_step, double trans_step);

struct EdgeMapConfig {
  types::Float pixel_uncertainty_match{2.0};
  types::Float match_threshold_norm{1.0};
  types::Float match_threshold_angle{45.0};
  types::Float regularization_threshold{0.5};
  using SharedPtr = std::shared_ptr<rebvio::EdgeMapConfig>;
};

class EdgeMap {
 public:
  using SharedPtr = std::shared_ptr<rebvio::EdgeMap>;

  // Reference signature (edge_map.hpp:34): an empty host-side map. Maps with keylines come from EdgeDetector::detect.
  EdgeMap(rebvio::Camera::SharedPtr camera, int size, uint64_t ts_us,
          rebvio::EdgeMapConfig::SharedPtr config = std::make_shared<rebvio::EdgeMapConfig>());
  ~EdgeMap();
  EdgeMap(const EdgeMap&) = delete;
  EdgeMap& operator=(const EdgeMap&) = delete;

  rebvio::types::KeyLine& operator[](int idx);
  int size();
  std::vector<rebvio::types::KeyLine>& keylines();
  uint64_t ts_us();
  const types::Float& threshold() const;
  void threshold(const types::Float& t);
  rebvio::types::IntegratedImu& imu();
  std::unordered_map<unsigned int, unsigned int>& mask();

  types::Float estimateQuantile(types::Float percentile, int num_bins);
  void rotateKeylines(const rebvio::types::Matrix3f& R);
  int forwardMatch(rebvio::EdgeMap::SharedPtr map);
  // One keyline of ANOTHER map searched in this one (reference edge_map.hpp:93-94); index of the match or -1.
  int searchMatch(const rebvio::types::KeyLine& keyline, const rebvio::types::Vector3f& vel, const rebvio::types::Matrix3f& Rvel,
                  const rebvio::types::Matrix3f& Rback, types::Float max_radius);
  int directedMatch(rebvio::EdgeMap::SharedPtr map, const rebvio::types::Vector3f& vel, const rebvio::types::Matrix3f& Rvel,
                    const rebvio::types::Matrix3f& Rback, int& kf_matches, types::Float max_radius);
  int regularize1Iter();
  // addition: the map's depth-bearing keylines as a point cloud, extracted on the device (rebvio_hip_map_point_cloud says
  // exactly which keylines and where; the synchronous form: it waits for everything queued that concerns this map)
  std::vector<rebvio::types::CloudPoint> pointCloud(const rebvio::types::CloudFilter& filter = rebvio::types::CloudFilter(),
                                                    const rebvio::types::CloudPose& pose = rebvio::types::CloudPose());
  // addition: the map's joined keylines as ordered edge chains and as 3D polylines (rebvio_hip_map_edge_chains /
  // rebvio_hip_map_edge_polylines define them; synchronous, from the tracking thread, like pointCloud). edgeChains: one record per
  // keyline, the keylines in chain order and the chains' first slots (starts.size() = chains + 1). edgePolylines: the kept slots as
  // points in slot order, {head, rank} per point, and one record per line.
  struct EdgeChains {
    std::vector<rebvio::types::ChainRef> refs;
    std::vector<int> order, starts;
  };
  struct EdgePolylines {
    std::vector<rebvio::types::CloudPoint> points;
    std::vector<std::array<int, 2>> refs;
    std::vector<rebvio::types::Polyline> lines;
  };
  EdgeChains edgeChains();
  EdgePolylines edgePolylines(const rebvio::types::PolylineOpts& opts = rebvio::types::PolylineOpts(),
                              const rebvio::types::CloudPose& pose = rebvio::types::CloudPose());
  // addition: the polylines split where they bend, each straight piece with two 3D end points whose depths are fitted to all of
  // its keylines (rebvio_hip_map_edge_segments defines it; synchronous, from the tracking thread, like edgePolylines). The kept
  // segments in point order and the counts of everything.
  struct EdgeSegments {
    std::vector<rebvio::types::LineSegment> segments;
    rebvio::types::SegmentCounts counts{};
  };
  EdgeSegments edgeSegments(const rebvio::types::SegmentOpts& opts = rebvio::types::SegmentOpts(),
                            const rebvio::types::CloudPose& pose = rebvio::types::CloudPose());
  // addition: a registered depth image folded into this map's rho / sigma_rho, one Kalman update per keyline
  // (rebvio_hip_map_fuse_depth_image defines it and says where in a stream it belongs: after the map has been a pair's new map -
  // or right after detection for a stream's first map - and before it serves as an old map; synchronous, from the tracking
  // thread, like pointCloud). The image is host memory of the context's size; image.unit > 0 replaces opts.unit. outcome: the
  // outcome word per keyline.
  rebvio::types::DepthPriorCounts fuseDepthImage(const rebvio::types::DepthImage& image,
                                                 const rebvio::types::DepthPriorOpts& opts = rebvio::types::DepthPriorOpts(),
                                                 std::vector<int>* outcome = nullptr);
  // addition: the edge map of the rectified right image of the same instant folded into this map's rho / sigma_rho: an epipolar
  // search in right's mask and one Kalman update per keyline (rebvio_hip_map_fuse_stereo defines it and says where in a stream it
  // belongs, as fuseDepthImage; synchronous, from the tracking thread). right: a map of this detector or of another one with the
  // same camera; it is only read. opts.baseline has no default. outcome / winner: the outcome word and the partner per keyline.
  rebvio::types::StereoPriorCounts fuseStereo(const EdgeMap& right, const rebvio::types::StereoPriorOpts& opts,
                                              std::vector<int>* outcome = nullptr, std::vector<int>* winner = nullptr);
  // addition: keyframes (rebvio_hip.h "Keyframes"). markKeyframe makes this map the keyframe: match_id_keyframe[i] = i for every
  // keyline, queued on the track stream - call it after the map has been a pair's new map and before it serves as an old map.
  // keyframeMatches(kf_size): which keylines of a keyframe of kf_size keylines live on in this map, in ascending kf_keyline
  // (synchronous, from the tracking thread, like pointCloud).
  void markKeyframe();
  std::vector<rebvio::types::KfMatch> keyframeMatches(int kf_size);
  // keyframeSnapshot keeps this map's keylines as they are now, in its own camera frame (queued on the track stream; take it where
  // the map is marked). keyframePose(snapshot): this map's pose relative to that keyframe, X_cur = R X_kf + t, estimated on the
  // device from the correspondences (rebvio_hip_map_keyframe_pose; synchronous, from the tracking thread). guess: the pose to
  // start from (its R and t; null: the identity), e.g. the previous result.
  rebvio::KeyframeSnapshot keyframeSnapshot();
  rebvio::types::KfPose keyframePose(const rebvio::KeyframeSnapshot& snapshot, const rebvio::types::KfPoseOpts& opts = rebvio::types::KfPoseOpts(),
                                     const rebvio::types::KfPose* guess = nullptr);
  // keyframeAlign(snapshot): the same pose, with the associations taken from THIS map's distance field instead of the
  // correspondence chain (rebvio_hip_map_keyframe_align; synchronous, from the tracking thread): any detected map of the
  // snapshot's context can be aligned, whatever has happened to the chain. assoc: per keyframe keyline the keyline of this map it
  // was associated with at the returned pose, or -1.
  rebvio::types::KfPose keyframeAlign(const rebvio::KeyframeSnapshot& snapshot, const rebvio::types::KfAlignOpts& opts = rebvio::types::KfAlignOpts(),
                                      const rebvio::types::KfPose* guess = nullptr, std::vector<int>* assoc = nullptr);

  // keyframeAlignMany(hypotheses): every (snapshot, guess) of the list aligned to THIS map in one set of launches
  // (rebvio_hip_map_keyframe_align_many; synchronous, from the tracking thread; 1..64 hypotheses, the same snapshot any number of
  // times). result[h].pose is keyframeAlign's for the same snapshot, guess and options, bit for bit; there are no associations: run
  // keyframeAlign on the winner (keyframeAlignBest) for them.
  std::vector<rebvio::types::KfHypResult> keyframeAlignMany(const std::vector<rebvio::types::KfHypothesis>& hypotheses,
                                                            const rebvio::types::KfAlignOpts& opts = rebvio::types::KfAlignOpts());

  // addition: place recognition (rebvio_hip.h "Place recognition"). placeSignature: 384 words, 8 x 6 image cells x 8 orientation
  // bins over the keylines this map holds now, normalised to 65535 (synchronous, from the tracking thread; take it where the map is
  // marked, as the snapshot: a map promised to the next pair's rotation is refused). counted: the keylines that entered it.
  // placeDb(capacity): a database of 1..65536 such signatures on this map's context.
  rebvio::types::PlaceSignature placeSignature(int* counted = nullptr) const;
  rebvio::PlaceDb placeDb(int capacity) const;

  // --- backend plumbing (not part of the reference surface) ---
  // `keepalive` owns the backend context the handle belongs to (backend::Session): a map kept by an edge-image consumer
  // (ros_rebvio.cpp:32-51) past ~Rebvio keeps its context alive and releases into it.
  void attach(rebvio_hip_ctx* ctx, rebvio_hip_map* handle, std::shared_ptr<void> keepalive = nullptr);
  rebvio_hip_map* handle() const { return handle_; }
  rebvio_hip_ctx* ctx() const { return ctx_; }
  void invalidateMirror() { mirror_valid_ = false; mask_valid_ = false; }

 private:
  void syncMirror();
  rebvio::EdgeMapConfig::SharedPtr config_;
  rebvio::Camera::SharedPtr camera_;
  uint64_t ts_us_;
  std::shared_ptr<void> keepalive_;  // declared before the handle: destroyed after the destructor body has released it
  rebvio_hip_ctx* ctx_ = nullptr;
  rebvio_hip_map* handle_ = nullptr;
  std::vector<rebvio::types::KeyLine> keylines_;
  std::unordered_map<unsigned int, unsigned int> keylines_mask_;
  bool mirror_valid_ = true, mask_valid_ = true;
  mutable types::Float threshold_;
  rebvio::types::IntegratedImu imu_;
};

}  // namespace rebvio
