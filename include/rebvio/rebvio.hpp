// rebvio::Rebvio — pipeline orchestrator with the reference's public surface (rebvio.hpp:38-62): two worker threads
// (edge detection || state estimation), image / IMU callbacks in, edge-image / odometry callbacks out.
// ros_rebvio.cpp builds against this header unchanged.
#pragma once

#include <atomic>
#include <functional>
#include <memory>
#include <mutex>
#include <deque>
#include <queue>
#include <thread>
#include <vector>

#include "rebvio/camera.hpp"
#include "rebvio/core.hpp"
#include "rebvio/edge_detector.hpp"
#include "rebvio/sab_estimator.hpp"
#include "rebvio/types/definitions.hpp"
#include "rebvio/types/depth_image.hpp"
#include "rebvio/types/image.hpp"
#include "rebvio/types/imu.hpp"
#include "rebvio/types/odometry.hpp"
#include "rebvio/types/place.hpp"
#include "rebvio/types/stereo_prior.hpp"
#include "rebvio/types/point_cloud.hpp"

namespace rebvio {

struct RebvioConfig {
  rebvio::EdgeDetectorConfig edge_detector;
  rebvio::CoreConfig core;
  rebvio::types::ImuStateConfig imu_state;
  rebvio::Camera camera;  // addition: the reference hard-codes EuRoC's camera; default-constructed = the same camera
  int device_id{0};       // addition: GPU ordinal of this camera stream
};

class Rebvio {
 public:
  Rebvio(rebvio::RebvioConfig& config);
  ~Rebvio();

  void imageCallback(rebvio::types::Image&& image);
  void imuCallback(rebvio::types::Imu&& imu);
  void registerEdgeImageCallback(std::function<void(cv::Mat&, rebvio::EdgeMap::SharedPtr&)> cb);
  void registerOdometryCallback(std::function<void(rebvio::types::Odometry&)> cb);
  // addition: the depth-bearing keylines of every published pair's new map as a point cloud (rebvio/types/point_cloud.hpp), in the
  // odometry's frame and metric: pose = R_global, Pos, K of the record. Called once per published odometry record, right after
  // the odometry callbacks, with the same ts_us, on the state-estimation thread; the points are valid during the call. The
  // cloud is extracted on the device behind the pair's second half and nobody waits for it before the pair's counters are
  // waited for anyway. While a callback is registered the next pair's first rotation is not fused into this pair's last kernel
  // (one launch more per pair); the odometry does not change by a digit. Register before the first frame is handed in.
  void registerPointCloudCallback(std::function<void(const rebvio::types::PointCloud&)> cb,
                                  rebvio::types::CloudFilter filter = rebvio::types::CloudFilter());
  // addition: the joined keylines of every published pair's new map as ordered 3D polylines (EdgeMap::edgePolylines;
  // rebvio_hip_map_edge_polylines defines a line), metric and in the odometry's frame with the pose of a point-cloud callback.
  // Called once per published odometry record, behind the point-cloud callbacks, on the state-estimation thread; the arrays are
  // valid during the call. The extraction is synchronous: the thread runs it behind the previous record's callbacks and waits for
  // this pair's second half there. As with a point-cloud callback the next pair's first rotation is then not fused into this
  // pair's last kernel; the odometry does not change by a digit. Without one the thread runs exactly the calls it ran. Register
  // before the first frame is handed in.
  void registerEdgePolylineCallback(std::function<void(const rebvio::types::EdgePolylines&)> cb,
                                    rebvio::types::PolylineOpts opts = rebvio::types::PolylineOpts());
  // addition: the straight segments of every published pair's new map (EdgeMap::edgeSegments; rebvio_hip_map_edge_segments defines
  // a segment and its fitted end depths), with the pose, the thread, the order (behind the polyline callbacks of the record) and
  // the rules of an edge-polyline callback: synchronous, the next pair's first rotation not fused into this pair's last kernel,
  // the odometry unchanged by a digit. Without one the thread runs exactly the calls it ran. Register before the first frame is
  // handed in.
  void registerEdgeSegmentCallback(std::function<void(const rebvio::types::EdgeSegments&)> cb,
                                   rebvio::types::SegmentOpts opts = rebvio::types::SegmentOpts());
  // addition: keyframes (rebvio_hip.h "Keyframes"). requestKeyframe: the newest tracked map becomes the keyframe - it is marked
  // (EdgeMap::markKeyframe) behind the second half of the pair being tracked when the request is seen, in front of the next pair's
  // first half; callable from any thread. The keyframe callback is called once per published odometry record, right after the
  // odometry callbacks, on the state-estimation thread: the record's stamp, kf_matches of its pair (keylines of the new map that
  // continue a keyline of the keyframe; 0 until a keyframe was requested) and the new map's keyline count - kf_matches / keylines
  // is the usual signal for requesting the next keyframe. With neither used the launches and the odometry are what they are
  // without them.
  void requestKeyframe() { keyframe_requested_ = true; }
  void registerKeyframeCallback(std::function<void(uint64_t ts_us, int kf_matches, int keylines)> cb);
  // addition: the pose of every tracked map relative to the keyframe, X_cur = R X_kf + t in keyframe depth units, estimated on the
  // device from the keyframe correspondences (EdgeMap::keyframePose; rebvio_hip.h defines it). While a pose callback is registered,
  // requestKeyframe also snapshots the keyframe right behind its mark (EdgeMap::keyframeSnapshot; the previous snapshot is dropped),
  // and from that pair on the state-estimation thread computes the new map's pose behind every pair's second half - warm-started
  // from the previous result, from the identity behind a new snapshot - and publishes it once per odometry record, right after the
  // keyframe callbacks: the record's stamp and the pose (the keyframe's own record carries the identity). As with a point-cloud
  // callback the next pair's first rotation is then not fused into this pair's last kernel, and the thread waits for the second
  // half before it goes on; the odometry does not change by a digit. Without one the thread runs exactly the calls it ran.
  // Register before the first frame is handed in.
  void registerKeyframePoseCallback(std::function<void(uint64_t ts_us, const rebvio::types::KfPose&)> cb);
  // addition: while this is on (default: off) and a keyframe-pose callback is registered, requestKeyframe also keeps the keyframe's
  // normals behind the snapshot (KeyframeSnapshot::addNormals) and the pose handed to the callback is the alignment of the snapshot
  // to the new map through the new map's distance field (EdgeMap::keyframeAlign; rebvio_hip.h defines it) instead of the pose from
  // the correspondence chain, warm-started exactly as that one is: it does not thin out with the chain. Off, the thread runs
  // exactly the calls it runs without this; the odometry does not change by a digit either way. Callable from any thread.
  void setKeyframeAlign(bool on) { keyframe_align_ = on; }
  // addition: while this is on (default: off), setKeyframeAlign is on and a keyframe-pose callback is registered, every new map
  // whose alignment came back with status 0 is fused into the snapshot at the returned pose (KeyframeSnapshot::fuseDepth;
  // rebvio_hip.h defines it): the keyframe's rho / sigma_rho tighten with every aligned view, and the next alignment solves against
  // them. The map the keyframe was marked on is not fused into itself. The counts go to the keyframe-fuse callbacks, once per such
  // record, right after the keyframe-pose callbacks, with the record's stamp. Off, the thread runs exactly the calls it runs
  // without this; the odometry does not change by a digit either way. Callable from any thread.
  void setKeyframeDepthFusion(bool on) { keyframe_depth_fusion_ = on; }
  void registerKeyframeFuseCallback(std::function<void(uint64_t ts_us, const rebvio::types::KfFuse&)> cb);
  // addition: hand a retiring keyframe's refined depths on to its successor. Default off; it acts only while setKeyframeAlign is on
  // and a keyframe-pose callback is registered, at a requestKeyframe mark that retires a snapshot whose last pose had status 0. The
  // outgoing snapshot is aligned to the newly marked map - behind the previous record's callbacks, warm-started from its last pose;
  // with a keyframe window it is the window's own result for its newest member, no second alignment - and on status 0
  // KeyframeSnapshot::handoverDepth writes its depths into the new snapshot where they are better than the tracker's raw ones
  // (rebvio_hip_kf_snapshot_handover_depth says exactly how; the two estimates are never combined). The mark's own keyframe-pose
  // record is computed in front of it and is what it is without the switch; the outgoing keyframe's cloud was queued earlier and
  // sees what it saw. The counts go to the keyframe-handover callbacks, once per hand-over, right after the keyframe-fuse callbacks:
  // the record's stamp, the outgoing keyframe's stamp, the counts. Off, the thread runs exactly the calls it runs without this; the
  // odometry does not change by a digit either way. Callable from any thread.
  void setKeyframeDepthHandover(bool on) { keyframe_depth_handover_ = on; }
  void registerKeyframeHandoverCallback(std::function<void(uint64_t ts_us, uint64_t kf_ts_us, const rebvio::types::KfHandover&)> cb);
  // addition: a window of the last n (0..15, default 0: none; values outside are clamped) retired keyframes. It is active only while
  // setKeyframeAlign is on and a keyframe-pose callback is registered. A keyframe that requestKeyframe retires - after its cloud has been
  // queued, so the keyframe-cloud callbacks see what they saw - then keeps its snapshot (and normals) and enters the window with its
  // stamp and its last status-0 pose, the oldest member leaving when there are more than n. Behind every pair the current keyframe AND
  // the members are aligned to the new map in ONE EdgeMap::keyframeAlignMany call (rebvio_hip.h defines it: the launches do not grow
  // with the members), each warm-started from its own last status-0 pose; a member whose result is not status 0 is reported once and
  // leaves. The pose handed to the keyframe-pose callbacks, and everything behind it (fusion, clouds), is the current keyframe's result:
  // bit for bit the pose of a run without a window. The keyframe-window callbacks get, once per such record and right after the
  // keyframe-fuse callbacks on the state-estimation thread, the record's stamp and one entry per aligned keyframe: the current one
  // first, then the members, newest first. With the window at 0 the thread runs exactly the calls it runs without this; the odometry
  // does not change by a digit either way. setKeyframeWindow is callable from any thread; register before the first frame is handed in.
  void setKeyframeWindow(int n) { keyframe_window_ = n < 0 ? 0 : (n > 15 ? 15 : n); }
  void registerKeyframeWindowCallback(std::function<void(uint64_t ts_us, const std::vector<rebvio::types::KfWindowPose>&)> cb);
  // addition: place recognition (rebvio/types/place.hpp, rebvio_hip.h "Place recognition"): notice that the camera has been here
  // before. Off at capacity 0, the default. On, the state-estimation thread keeps a PlaceDb of `capacity` (1..65536) signatures: at
  // every requestKeyframe mark, right behind the snapshot, it queries the database with the marked map (EdgeMap::placeSignature's
  // 384 words against every entry but the last exclude_last, the top_k <= 16 nearest) and then adds the map with tag = the
  // keyframe's stamp. A full database stops adding and counts the misses (placeMisses). The place callback gets the record's stamp
  // and the matches with distance <= max_distance, nearest first - possibly none - once per mark, on the state-estimation thread,
  // after the other keyframe callbacks of the record. The matches are candidates, not poses: their tags say which keyframes to
  // hand to EdgeMap::keyframeAlignMany. max_distance = 32768 is a choice, a quarter of the largest distance two normalised
  // signatures can have, not a measurement on real footage (INTEGRATION.md "Places"). A marked map is not handed to the next
  // pair's rotation early (as with a keyframe-pose callback); on or off the odometry does not change by a digit, and off the
  // thread runs exactly the calls it runs without this. Call both before the first frame is handed in.
  void setPlaceRecognition(int capacity, int top_k = 4, int exclude_last = 10, uint32_t max_distance = 32768);
  void registerPlaceCallback(std::function<void(uint64_t ts_us, const std::vector<rebvio::types::PlaceMatch>&)> cb);
  unsigned int placeQueries() const { return place_queries_; }
  unsigned int placeMatches() const { return place_matches_; }
  unsigned int placeMisses() const { return place_misses_; }
  // addition: every keyframe's depth-bearing keylines as one point cloud, handed out as the keyframe is retired
  // (KeyframeSnapshot::pointCloud; rebvio_hip.h defines it). While such a callback is registered requestKeyframe snapshots the
  // keyframe behind its mark as a keyframe-pose callback makes it do, and remembers R_global, Pos, K of the odometry record of the map
  // it was marked on. The next requestKeyframe replaces that snapshot; before it does, the outgoing keyframe's cloud is queued on the
  // device with that remembered pose - metric and in the odometry's frame, like the per-map clouds - and it is delivered with the
  // record of the pair whose new map takes over as keyframe (the next record published), right after the other keyframe callbacks,
  // on the state-estimation thread: ts_us is the retired keyframe's own stamp, pose the remembered one, `keyline` the index in the
  // keyframe, gradient_norm 0; the points are valid during the call. One cloud per retired keyframe is the unit a mapping consumer
  // concatenates. With setKeyframeAlign and setKeyframeDepthFusion on (and the keyframe-pose callback they need) it is the refined
  // keyframe, every aligned view folded in; without them the keyframe as marked. The keyframe that is still current when
  // processing ends is not handed out: one more requestKeyframe before the last frames retires it. As with a point-cloud callback
  // the next pair's first rotation is then not fused into this pair's last kernel; the odometry does not change by a digit.
  // Without one the thread runs exactly the calls it ran. Register before the first frame is handed in.
  void registerKeyframeCloudCallback(std::function<void(const rebvio::types::PointCloud&)> cb,
                                     rebvio::types::CloudFilter filter = rebvio::types::CloudFilter());
  // addition: registered depth images (RGB-D; rebvio/types/depth_image.hpp, rebvio_hip.h "Depth prior from a registered depth
  // image"). depthImageCallback copies the image into a small queue (at most 8; a ninth pushes the oldest out, counted as dropped);
  // callable from any thread - hand it in AHEAD of the imageCallback of the same stamp: an image that arrives after its frame's pair
  // has been started is never matched and ends as dropped. The state-estimation thread matches an
  // image to the frame with the SAME ts_us: the image of a pair's new map is folded into that map's rho / sigma_rho by a kernel
  // queued right behind the pair's second half (the thread does not wait for it), the image of a stream's first map in front of its
  // first pair; from then on the map's depths, V and the position are metric through the prior. An image older than the frame being
  // tracked is dropped and counted (depthImagesDropped). While an image is waiting for the pair's new map the next pair's first
  // rotation is not fused into this pair's last kernel, as with a point-cloud callback. A frame without an image runs exactly the
  // calls it runs without all this. setDepthPrior: the options of the fusions queued from then on (any thread). The depth-prior
  // callback gets the frame's stamp and the counts, once per fused frame, behind the odometry callbacks of the record published
  // next (for the first map: in front of the first record's other callbacks), on the state-estimation thread.
  void depthImageCallback(rebvio::types::DepthImage&& image);
  void setDepthPrior(const rebvio::types::DepthPriorOpts& opts);
  void registerDepthPriorCallback(std::function<void(uint64_t ts_us, const rebvio::types::DepthPriorCounts&)> cb);
  unsigned int depthImagesDropped() const { return depth_dropped_; }
  // addition: a rectified stereo partner (rebvio/types/stereo_prior.hpp, rebvio_hip.h "Depth prior from a rectified stereo
  // partner"). setStereo makes a second, detect-only EdgeDetector with the left one's camera and parameters (a backend context
  // of its own: the right camera gets its own threshold servo) and sets the options of the fusions queued from then on; call it
  // before the first right image. rightImageCallback queues the image (at most 8; a ninth pushes the oldest out, counted as
  // dropped); callable from any thread - hand it in AHEAD of the imageCallback of the same stamp. The right frames are assumed
  // rectified to the left ones. The state-estimation thread matches an image to the left frame with the SAME ts_us, detects it and
  // queues the fusion into that frame's map right behind the pair's second half, as a depth image (for a stream's first map: in
  // front of its first pair); with a depth image for the same frame the depth image goes first. Older images are dropped and
  // counted (rightImagesDropped). A frame without a partner runs exactly the calls it runs without all this. The stereo-prior
  // callback gets the frame's stamp and the counts, once per fused frame, where the depth-prior callback gets its own.
  void setStereo(const rebvio::types::StereoPriorOpts& opts);
  void rightImageCallback(rebvio::types::Image&& image);
  void registerStereoPriorCallback(std::function<void(uint64_t ts_us, const rebvio::types::StereoPriorCounts&)> cb);
  unsigned int rightImagesDropped() const { return right_dropped_; }
  // addition: detection mask (EdgeDetector::setDetectionMask) for the frames handed to imageCallback after this call; frames
  // queued before it keep the mask they were queued with. Safe while the worker threads run. An empty Mat clears it.
  void setDetectionMask(const cv::Mat& mask);

  // additions for embedding without ROS: block until every queued frame has been processed / current status
  void waitIdle();
  bool running() const { return run_; }
  unsigned int framesProcessed() const { return num_frames_; }

 private:
  void dataAcquisitionProcess();
  void stateEstimationProcess();

  rebvio::RebvioConfig config_;
  std::atomic<bool> run_;
  std::atomic<unsigned int> num_frames_, num_detected_, num_images_, num_published_{0};
  rebvio::Camera camera_;
  rebvio::EdgeDetector edge_detector_;
  rebvio::Core core_;
  rebvio::types::ImuState imu_state_;
  rebvio::SABEstimator::State sab_state_;  // after core_ and config_ in construction order

  std::queue<rebvio::types::Image> image_buffer_;
  std::queue<std::shared_ptr<const cv::Mat>> image_mask_buffer_;  // the detection mask of each queued image (null: none)
  std::shared_ptr<const cv::Mat> mask_;                          // ... for the images queued next (under image_buffer_mutex_)
  std::mutex image_buffer_mutex_;
  std::queue<rebvio::types::Imu> imu_buffer_;
  std::mutex imu_buffer_mutex_;
  std::deque<rebvio::EdgeMap::SharedPtr> edge_map_buffer_;  // (a deque: the tracker looks one map ahead for the next pair's gyro prior)
  std::mutex edge_map_buffer_mutex_;
  std::vector<std::function<void(cv::Mat&, rebvio::EdgeMap::SharedPtr&)>> edge_image_callbacks_;
  std::vector<std::function<void(rebvio::types::Odometry&)>> odometry_callbacks_;
  struct PointCloudCallback {
    std::function<void(const rebvio::types::PointCloud&)> cb;
    rebvio::types::CloudFilter filter;
  };
  std::vector<PointCloudCallback> point_cloud_callbacks_;
  std::vector<PointCloudCallback> keyframe_cloud_callbacks_;
  struct EdgePolylineCallback {
    std::function<void(const rebvio::types::EdgePolylines&)> cb;
    rebvio::types::PolylineOpts opts;
  };
  std::vector<EdgePolylineCallback> edge_polyline_callbacks_;
  struct EdgeSegmentCallback {
    std::function<void(const rebvio::types::EdgeSegments&)> cb;
    rebvio::types::SegmentOpts opts;
  };
  std::vector<EdgeSegmentCallback> edge_segment_callbacks_;
  std::vector<std::function<void(uint64_t, int, int)>> keyframe_callbacks_;
  std::vector<std::function<void(uint64_t, const rebvio::types::KfPose&)>> keyframe_pose_callbacks_;
  std::vector<std::function<void(uint64_t, const std::vector<rebvio::types::PlaceMatch>&)>> place_callbacks_;
  std::atomic<int> place_capacity_{0}, place_top_k_{4}, place_exclude_last_{10};
  std::atomic<uint32_t> place_max_distance_{32768};
  std::atomic<unsigned int> place_queries_{0}, place_matches_{0}, place_misses_{0};
  std::atomic<bool> keyframe_requested_{false};
  std::atomic<bool> keyframe_align_{false};
  std::vector<std::function<void(uint64_t, const rebvio::types::KfFuse&)>> keyframe_fuse_callbacks_;
  std::atomic<bool> keyframe_depth_fusion_{false};
  std::vector<std::function<void(uint64_t, uint64_t, const rebvio::types::KfHandover&)>> keyframe_handover_callbacks_;
  std::atomic<bool> keyframe_depth_handover_{false};
  std::vector<std::function<void(uint64_t, const std::vector<rebvio::types::KfWindowPose>&)>> keyframe_window_callbacks_;
  std::atomic<int> keyframe_window_{0};
  // depth images: the queue (under depth_mutex_, with the options), what the state-estimation thread keeps on the device for the
  // queued fusions (two staging frames, used in turn: a frame's image is uploaded while the previous one may still be read)
  struct QueuedDepth {
    uint64_t ts_us;
    int format;
    double unit;
    std::vector<unsigned char> bytes;  // dense rows
  };
  std::deque<QueuedDepth> depth_queue_;
  rebvio::types::DepthPriorOpts depth_opts_;
  std::mutex depth_mutex_;
  std::atomic<unsigned int> depth_seen_{0}, depth_dropped_{0};
  std::vector<std::function<void(uint64_t, const rebvio::types::DepthPriorCounts&)>> depth_prior_callbacks_;
  void* depth_dev_[2] = {nullptr, nullptr};
  unsigned int depth_dev_turn_ = 0;
  // the stereo partner: its detector (setStereo), the queue of right images (under stereo_mutex_, with the options), and the two
  // right maps the queued fusions may still read, kept in turn
  std::unique_ptr<rebvio::EdgeDetector> right_detector_;
  std::deque<rebvio::types::Image> right_queue_;
  rebvio::types::StereoPriorOpts stereo_opts_;
  std::mutex stereo_mutex_;
  std::atomic<unsigned int> right_seen_{0}, right_dropped_{0};
  std::vector<std::function<void(uint64_t, const rebvio::types::StereoPriorCounts&)>> stereo_prior_callbacks_;
  rebvio::EdgeMap::SharedPtr right_hold_[2];
  unsigned int right_hold_turn_ = 0;
  std::thread data_acquisition_thread_, state_estimation_thread_;
};

}  // namespace rebvio
