// rebvio::Rebvio over the gfx950 backend. Same threading model and observable behaviour as the reference
// (rebvio.cpp:17-313): the caller thread converts/undistorts and queues images; worker 1 detects edges and attaches the
// pre-integrated IMU data; worker 2 runs one tracking step per frame pair and publishes odometry.
//
// The frame-pair step is calls into the backend with the O(1) inertial fusion between them (and the previous pair's
// counters fetched while this pair's first half is already queued behind that pair's second half, so that the GPU goes from
// one pair to the next without waiting for the host):
//   rebvio_hip_track_pair_begin  - distance field, rotate by the gyro prior, minimizeVel, forwardMatch, extRotVel,
//                                  gyroBiasCorrection (rebvio.cpp:142-192)
//   host                         - Ls4 / mean acceleration, Core::estimateBias + SABEstimator, second rotation
//                                  (rebvio.cpp:195-233)
//   rebvio_hip_track_pair_finish_async / _result - rotate, directedMatch, regularize, depth EKF (rebvio.cpp:222-259)
// followed by the gravity-aligned pose integration (rebvio.cpp:263-271). The reference's latent races (unlocked queue
// peeks, plain-bool run flag) are not inherited.
#include "rebvio/rebvio.hpp"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>

#include "../csrc/hostmath.hpp"
#include "../csrc/pixel_format.hpp"
#include "rebvio/util/log.hpp"
#include "session.hpp"

namespace rebvio {

namespace {
struct ScopeOpener {  // runs before the detector/tracker members are constructed
  explicit ScopeOpener(int device) { backend::Session::newScope(device); }
};

// The reference library throws nothing from its workers: a failed step prints to stderr and clears run_
// (rebvio.cpp:236-252). A backend error surfacing on a worker thread (edge-map pool exhausted, a HIP failure) does the
// same here instead of ending the process through std::terminate.
template <class Body>
void run_worker(const char* name, std::atomic<bool>& run, Body&& body) {
  try {
    body();
  } catch (const std::exception& e) {
    std::cerr << name << " stopped: " << e.what() << "\n";
    run = false;
  } catch (...) {
    std::cerr << name << " stopped: unknown error\n";
    run = false;
  }
}
}  // namespace

Rebvio::Rebvio(rebvio::RebvioConfig& config)
    : config_((ScopeOpener(config.device_id), config)), run_(true), num_frames_(0), num_detected_(0), num_images_(0),
      camera_(config.camera),
      edge_detector_(std::make_shared<rebvio::Camera>(camera_), std::make_shared<rebvio::EdgeDetectorConfig>(config.edge_detector)),
      core_(std::make_shared<rebvio::Camera>(camera_), std::make_shared<rebvio::CoreConfig>(config.core)),
      sab_state_(config_.imu_state) {
  core_.session()->setImuNoise(config_.imu_state.gyro_std_dev, config_.imu_state.gyro_bias_std_dev);
  core_.session()->ctx();  // create the device context now: fail loudly here, not in a worker thread
  data_acquisition_thread_ = std::thread([this] { run_worker("Data Acquisition Process", run_, [this] { dataAcquisitionProcess(); }); });
  state_estimation_thread_ = std::thread([this] { run_worker("State Estimation Process", run_, [this] { stateEstimationProcess(); }); });
}

Rebvio::~Rebvio() {
  run_ = false;
  if (data_acquisition_thread_.joinable()) data_acquisition_thread_.join();
  if (state_estimation_thread_.joinable()) state_estimation_thread_.join();
  for (void*& p : depth_dev_)  // the depth images' device staging frames (the workers have ended: nothing reads them)
    if (p) {
      (void)rebvio_hip_device_free(core_.session()->ctx(), p);
      p = nullptr;
    }
}

void Rebvio::depthImageCallback(rebvio::types::DepthImage&& image) {
  if (!image.data || (image.format != types::DEPTH_U16 && image.format != types::DEPTH_F32) || image.rows != (int)camera_.rows_ ||
      image.cols != (int)camera_.cols_)
    backend::fail("Rebvio::depthImageCallback: the depth image must be DEPTH_U16 or DEPTH_F32 of the camera's size", -3);
  const size_t rowb = (size_t)image.cols * (image.format == types::DEPTH_U16 ? 2 : 4), pitch = image.pitch ? image.pitch : rowb;
  if (pitch < rowb) backend::fail("Rebvio::depthImageCallback: pitch below a row's bytes", -3);
  QueuedDepth q{image.ts_us, image.format, image.unit, std::vector<unsigned char>((size_t)image.rows * rowb)};
  for (int r = 0; r < image.rows; ++r)
    std::memcpy(q.bytes.data() + (size_t)r * rowb, static_cast<const unsigned char*>(image.data) + (size_t)r * pitch, rowb);
  std::lock_guard<std::mutex> guard(depth_mutex_);
  if (depth_queue_.size() >= 8) {
    depth_queue_.pop_front();
    ++depth_dropped_;
  }
  depth_queue_.push_back(std::move(q));
  ++depth_seen_;
}

void Rebvio::setDepthPrior(const rebvio::types::DepthPriorOpts& opts) {
  std::lock_guard<std::mutex> guard(depth_mutex_);
  depth_opts_ = opts;
}

void Rebvio::registerDepthPriorCallback(std::function<void(uint64_t ts_us, const rebvio::types::DepthPriorCounts&)> cb) {
  depth_prior_callbacks_.push_back(cb);
}

void Rebvio::setStereo(const rebvio::types::StereoPriorOpts& opts) {
  std::lock_guard<std::mutex> guard(stereo_mutex_);
  stereo_opts_ = opts;
  if (!right_detector_) {
    backend::Session::newScope(config_.device_id);  // a context of its own: the right camera's threshold servo is not the left one's
    right_detector_ = std::make_unique<rebvio::EdgeDetector>(std::make_shared<rebvio::Camera>(camera_),
                                                             std::make_shared<rebvio::EdgeDetectorConfig>(config_.edge_detector));
  }
}

void Rebvio::rightImageCallback(rebvio::types::Image&& image) {
  if (image.data.rows != (int)camera_.rows_ || image.data.cols != (int)camera_.cols_)
    backend::fail("Rebvio::rightImageCallback: the image must have the camera's size", -3);
  rebvio::types::Image q;
  q.ts_us = image.ts_us;
  const int t = image.data.type();
  if (t != CV_8UC1 && t != CV_8UC3 && t != CV_8UC4) {
    cv::Mat img;
    image.data.convertTo(img, CV_FLOAT_PRECISION, 3.0);
    q.data = camera_.undistort(img);
  } else {
    q.data = image.data.clone();  // (the caller's buffer may be reused before the frame's pair comes up)
  }
  std::lock_guard<std::mutex> guard(stereo_mutex_);
  if (!right_detector_) backend::fail("Rebvio::rightImageCallback: call setStereo first", -3);
  if (right_queue_.size() >= 8) {
    right_queue_.pop_front();
    ++right_dropped_;
  }
  right_queue_.push_back(std::move(q));
  ++right_seen_;
}

void Rebvio::registerStereoPriorCallback(std::function<void(uint64_t ts_us, const rebvio::types::StereoPriorCounts&)> cb) {
  stereo_prior_callbacks_.push_back(cb);
}

void Rebvio::setPlaceRecognition(int capacity, int top_k, int exclude_last, uint32_t max_distance) {
  if (capacity < 0 || capacity > 65536) backend::fail("Rebvio::setPlaceRecognition: capacity outside 0..65536", -3);
  if (top_k < 1 || top_k > types::kPlaceTopKMax) backend::fail("Rebvio::setPlaceRecognition: top_k outside 1..16", -3);
  if (exclude_last < 0) backend::fail("Rebvio::setPlaceRecognition: negative exclude_last", -3);
  place_top_k_ = top_k;
  place_exclude_last_ = exclude_last;
  place_max_distance_ = max_distance;
  place_capacity_ = capacity;
}

void Rebvio::registerPlaceCallback(std::function<void(uint64_t ts_us, const std::vector<rebvio::types::PlaceMatch>&)> cb) {
  place_callbacks_.push_back(cb);
}

void Rebvio::imageCallback(rebvio::types::Image&& image) {
  std::lock_guard<std::mutex> guard(image_buffer_mutex_);
  const int t = image.data.type();
  if (t != CV_8UC1 && t != CV_8UC3 && t != CV_8UC4) {
    // not an 8-bit frame: convert and undistort here like the reference does (rebvio.cpp:43-47)
    cv::Mat img;
    image.data.convertTo(img, CV_FLOAT_PRECISION, 3.0);  // 0..765, matches max_image_value_ (edge_detector.cpp:21)
    image.data = camera_.undistort(img);
  }  // else: the u8 frame (MONO8, BGR8 or BGRA8) goes to the device as it is; grey conversion, x3 and undistort run there
  image_buffer_.push(image);
  image_mask_buffer_.push(mask_);
  ++num_images_;
}

void Rebvio::setDetectionMask(const cv::Mat& mask) {
  std::shared_ptr<const cv::Mat> m;
  if (!mask.empty()) {
    if (mask.type() != CV_8UC1 || mask.rows != (int)camera_.rows_ || mask.cols != (int)camera_.cols_)
      backend::fail("Rebvio::setDetectionMask: the mask must be CV_8UC1 of the camera's size", -1);
    m = std::make_shared<const cv::Mat>(mask.clone());
  }
  // the acquisition thread hands it to the detector in front of the first frame queued from here on
  std::lock_guard<std::mutex> guard(image_buffer_mutex_);
  mask_ = m;
}

void Rebvio::imuCallback(rebvio::types::Imu&& imu) {
  std::lock_guard<std::mutex> guard(imu_buffer_mutex_);
  imu_buffer_.push(imu);
}

void Rebvio::registerEdgeImageCallback(std::function<void(cv::Mat&, rebvio::EdgeMap::SharedPtr&)> cb) {
  edge_image_callbacks_.push_back(cb);
}

void Rebvio::registerOdometryCallback(std::function<void(rebvio::types::Odometry&)> cb) { odometry_callbacks_.push_back(cb); }

void Rebvio::registerKeyframeWindowCallback(std::function<void(uint64_t ts_us, const std::vector<rebvio::types::KfWindowPose>&)> cb) {
  keyframe_window_callbacks_.push_back(cb);
}
void Rebvio::registerKeyframeCallback(std::function<void(uint64_t ts_us, int kf_matches, int keylines)> cb) { keyframe_callbacks_.push_back(cb); }

void Rebvio::registerKeyframePoseCallback(std::function<void(uint64_t ts_us, const rebvio::types::KfPose&)> cb) {
  keyframe_pose_callbacks_.push_back(cb);
}

void Rebvio::registerKeyframeFuseCallback(std::function<void(uint64_t ts_us, const rebvio::types::KfFuse&)> cb) {
  keyframe_fuse_callbacks_.push_back(cb);
}

void Rebvio::registerKeyframeHandoverCallback(std::function<void(uint64_t ts_us, uint64_t kf_ts_us, const rebvio::types::KfHandover&)> cb) {
  keyframe_handover_callbacks_.push_back(cb);
}

void Rebvio::registerEdgePolylineCallback(std::function<void(const rebvio::types::EdgePolylines&)> cb, rebvio::types::PolylineOpts opts) {
  edge_polyline_callbacks_.push_back({cb, opts});
}

void Rebvio::registerEdgeSegmentCallback(std::function<void(const rebvio::types::EdgeSegments&)> cb, rebvio::types::SegmentOpts opts) {
  edge_segment_callbacks_.push_back({cb, opts});
}

void Rebvio::registerPointCloudCallback(std::function<void(const rebvio::types::PointCloud&)> cb, rebvio::types::CloudFilter filter) {
  point_cloud_callbacks_.push_back({cb, filter});
}

void Rebvio::registerKeyframeCloudCallback(std::function<void(const rebvio::types::PointCloud&)> cb, rebvio::types::CloudFilter filter) {
  keyframe_cloud_callbacks_.push_back({cb, filter});
}

void Rebvio::waitIdle() {
  while (run_) {
    const unsigned imgs = num_images_;
    if (num_detected_ >= imgs && (imgs < 2 || num_published_ + 1 >= imgs)) return;
    std::this_thread::sleep_for(std::chrono::milliseconds(1));
  }
}

void Rebvio::dataAcquisitionProcess() {
  REBVIO_INFO("Starting Data Acquisition Process..");
  std::shared_ptr<const cv::Mat> mask_set;  // the detection mask the detector has now
  while (run_) {
    rebvio::types::Image img;
    std::shared_ptr<const cv::Mat> mask;
    bool have = false;
    {
      std::lock_guard<std::mutex> guard(image_buffer_mutex_);
      if (!image_buffer_.empty()) {
        img = image_buffer_.front();
        image_buffer_.pop();
        mask = image_mask_buffer_.front();
        image_mask_buffer_.pop();
        have = true;
      }
    }
    if (!have) {
      std::this_thread::sleep_for(std::chrono::milliseconds(1));
      continue;
    }
    // back-pressure: the reference's edge-map queue is unbounded (rebvio.cpp:86-90); here every queued map holds device
    // memory from a bounded pool, so detection waits while the tracker is more than a few maps behind
    for (;;) {
      size_t queued;
      {
        std::lock_guard<std::mutex> guard(edge_map_buffer_mutex_);
        queued = edge_map_buffer_.size();
      }
      if (queued < 8 || !run_) break;
      std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
    if (mask != mask_set) {  // (this thread launches every detection: the frames detected so far keep their mask)
      edge_detector_.setDetectionMask(mask ? *mask : cv::Mat());
      mask_set = mask;
    }
    static const bool acq_timers = std::getenv("REBVIO_HOST_TIMERS") != nullptr;
    const auto td0 = std::chrono::steady_clock::now();
    rebvio::EdgeMap::SharedPtr edge_map = edge_detector_.detect(img);
    if (acq_timers) {
      static double acc_us = 0;
      static unsigned acc_n = 0;
      acc_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - td0).count();
      if (++acc_n % 2000 == 0) std::fprintf(stderr, "[Rebvio] EdgeDetector::detect (staging + enqueue) %.1f us per frame on the acquisition thread\n", acc_us / acc_n);
    }
    if (!edge_image_callbacks_.empty()) {
      // callbacks see the undistorted frame, as in the reference; for a raw u8 frame of a distorting lens it is fetched
      // from the device front end (only when somebody listens). A colour frame gives what its grey frame would: the device
      // front end's output with a lens model, else the CV_8UC1 grey frame of the host form of the conversion.
      const int t = img.data.type();
      const int fmt = t == CV_8UC3 ? REBVIO_HIP_PX_BGR8 : t == CV_8UC4 ? REBVIO_HIP_PX_BGRA8 : REBVIO_HIP_PX_GRAY8;
      if (t == CV_8UC1 && core_.session()->hasDistortion()) {
        cv::Mat und(img.data.rows, img.data.cols, CV_32FC1);
        cv::Mat dense = (img.data.step == (size_t)img.data.cols) ? img.data : img.data.clone();
        backend::check("rebvio_hip_front_end_u8",
                       rebvio_hip_front_end_u8(core_.session()->ctx(), dense.ptr<unsigned char>(0), und.ptr<float>(0)));
        img.data = und;
      } else if (fmt != REBVIO_HIP_PX_GRAY8 && core_.session()->hasDistortion()) {
        cv::Mat und(img.data.rows, img.data.cols, CV_32FC1);
        backend::check("rebvio_hip_front_end_px", rebvio_hip_front_end_px(core_.session()->ctx(), img.data.ptr<unsigned char>(0),
                                                                          img.data.step, fmt, und.ptr<float>(0)));
        img.data = und;
      } else if (fmt != REBVIO_HIP_PX_GRAY8) {
        cv::Mat grey(img.data.rows, img.data.cols, CV_8UC1);
        rh::px::to_grey(fmt, img.data.ptr<unsigned char>(0), img.data.step, img.data.rows, img.data.cols, grey.ptr<unsigned char>(0));
        img.data = grey;
      }
      for (auto& cb : edge_image_callbacks_) cb(img.data, edge_map);
    }
    {
      // integrate the IMU samples up to this frame BEFORE the map becomes visible to the tracker
      std::lock_guard<std::mutex> guard(imu_buffer_mutex_);
      while (!imu_buffer_.empty() && imu_buffer_.front().ts <= img.ts_us) {
        edge_map->imu().add(imu_buffer_.front(), camera_.getRc2i());
        imu_buffer_.pop();
      }
    }
    {
      std::lock_guard<std::mutex> guard(edge_map_buffer_mutex_);
      edge_map_buffer_.push_back(edge_map);
    }
    ++num_detected_;
  }
}

namespace {
// stand-in for the reference's REBVIO_TIMER accumulators (util/timer.hpp): per-stage host times of the tracking worker,
// printed when the worker ends if REBVIO_HOST_TIMERS is set
struct StageTimers {
  bool on = std::getenv("REBVIO_HOST_TIMERS") != nullptr;
  double t[4] = {0, 0, 0, 0};
  double t_bias = 0;  // Core::estimateBias alone (inside t[1])
  double t_in = 0;  // from the end of a pair to the next pair's first device call (input queue, IMU pre-integration read)
  std::chrono::steady_clock::time_point pair_end;
  bool have_end = false;
  unsigned n = 0;
  std::chrono::steady_clock::time_point last;
  void start() {
    if (!on) return;
    last = std::chrono::steady_clock::now();
    if (have_end) t_in += std::chrono::duration<double, std::micro>(last - pair_end).count();
  }
  void end_pair() {
    if (!on) return;
    pair_end = std::chrono::steady_clock::now();
    have_end = true;
  }
  void lap(int i) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    t[i] += std::chrono::duration<double, std::micro>(now - last).count();
    last = now;
  }
  ~StageTimers() {
    if (on && n)
      std::fprintf(stderr, "[Rebvio] per pair (us): first half on device %.1f  acceleration + bias/scale filter %.1f  second half on device %.1f  pose + callbacks %.1f  (between pairs: input queue + IMU read %.1f)\n",
                   t[0] / n, t[1] / n, t[2] / n, t[3] / n, t_in / n);
    const backend::FusionCounters& f = backend::t_fusion;
    if (on && n && f.gn_calls)
      std::fprintf(stderr, "[Rebvio]   estimateBias %.1f us per pair: %.2f Gauss-Newton iterations per call, %lu of %lu solves through the pseudo-inverse\n",
                   t_bias / n, (double)f.gn_iterations / f.gn_calls, f.pinv_solves, f.gn_iterations);
  }
};
// REBVIO_DUMP_FUSION=<file>: every Core::estimateBias call of the run as 237 raw floats - 100 inputs (sacc, facc, kP, Rot, Qg,
// Qrot, Qbias, QKp, Rg, g_norm, Rs, Rf, Wvw), the 68 state words (X, P, g_est, b_est, Xvw) before the call, the scale it
// returned and the state words after it. tests/golden/estimate_bias_calls.npz was recorded this way
// (tools/record_fusion_calls.py); tests/test_fusion_math.py replays it on the CPU.
struct FusionDump {
  FILE* f = std::getenv("REBVIO_DUMP_FUSION") ? std::fopen(std::getenv("REBVIO_DUMP_FUSION"), "wb") : nullptr;
  void put(float v) { std::fwrite(&v, 4, 1, f); }
  void put3(const types::Matrix3f& m) {
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) put(m(i, j));
  }
  void state(const SABEstimator::State& s, const types::Vector6f& Xvw) {
    for (int i = 0; i < 7; ++i) put(s.X[i]);
    for (int i = 0; i < 7; ++i)
      for (int j = 0; j < 7; ++j) put(s.P(i, j));
    for (int i = 0; i < 3; ++i) put(s.g_est[i]);
    for (int i = 0; i < 3; ++i) put(s.b_est[i]);
    for (int i = 0; i < 6; ++i) put(Xvw[i]);
  }
  void before(const types::Vector3f& sacc, const types::Vector3f& facc, float kP, const types::Matrix3f& Rot,
              const SABEstimator::State& s, const types::Matrix6f& Wvw, const types::Vector6f& Xvw, float g_norm) {
    if (!f) return;
    for (int i = 0; i < 3; ++i) put(sacc[i]);
    for (int i = 0; i < 3; ++i) put(facc[i]);
    put(kP);
    put3(Rot);
    put3(s.Qg);
    put3(s.Qrot);
    put3(s.Qbias);
    put(s.QKp);
    put(s.Rg);
    put(g_norm);
    put3(s.Rs);
    put3(s.Rv);
    for (int i = 0; i < 6; ++i)
      for (int j = 0; j < 6; ++j) put(Wvw(i, j));
    state(s, Xvw);
  }
  void after(float k, const SABEstimator::State& s, const types::Vector6f& Xvw) {
    if (!f) return;
    put(k);
    state(s, Xvw);
  }
  ~FusionDump() {
    if (f) std::fclose(f);
  }
};
}  // namespace

void Rebvio::stateEstimationProcess() {
  REBVIO_INFO("Starting State Estimation Process..");
  StageTimers timers;
  FusionDump fusion_dump;
  rebvio_hip_ctx* ctx = core_.session()->ctx();
  const types::Float FMAX = std::numeric_limits<types::Float>::max();
  types::Vector3f Pos = TooN::Zeros;
  types::Matrix3f R_global = TooN::Identity;
  types::Float K = 1.0;
  types::Float P_Kp = 5e-6;
  int num_gyro_init = 0;
  types::Vector3f gyro_init = TooN::Zeros;
  types::Vector3f g_init = TooN::Zeros;

  auto load3 = [](const float* p) {
    types::Matrix3f m;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) m(i, j) = p[i * 3 + j];
    return m;
  };
  auto store3 = [](const types::Matrix3f& m, float* p) {
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) p[i * 3 + j] = m(i, j);
  };

  // The odometry of a pair is complete once its second half has reported its match count (rebvio.cpp:245-252). That is
  // fetched AFTER the next pair's first half has been queued, so the record waits here for one loop turn (or until the
  // input runs dry). Returns false when the pair ended the run (minimization error / too few matches).
  struct Pending {
    bool have = false;     // a pair whose counters have not been fetched yet
    bool fetched = false;  // counters in, record not yet handed to the callbacks
    types::Odometry odometry;
    rebvio::EdgeMap::SharedPtr old_map, new_map;
    // point-cloud callbacks: the pose the pair's clouds were queued with and one queued cloud per callback (waited for where
    // the pair's counters are)
    types::CloudPose cloud_pose;
    std::vector<rebvio_hip_cloud*> clouds;
    // keyframe-cloud callbacks: the cloud of the keyframe this pair's new map replaced, one queued cloud per callback, with the
    // stamp and the pose remembered where that keyframe was marked
    std::vector<rebvio_hip_cloud*> kf_clouds;
    types::CloudPose kf_cloud_pose;
    uint64_t kf_cloud_ts = 0;
    int kf_matches = 0;    // of the pair, for the keyframe callbacks
    bool have_kf_pose = false;  // keyframe-pose callbacks: the new map's pose relative to the keyframe
    types::KfPose kf_pose;
    bool have_kf_fuse = false;  // setKeyframeDepthFusion: the counts of the new map's fusion into the snapshot
    types::KfFuse kf_fuse;
    bool have_kf_handover = false;  // setKeyframeDepthHandover: the counts of the retired keyframe's hand-over into the new snapshot
    types::KfHandover kf_handover;
    uint64_t kf_handover_ts = 0;    // ... and the retired keyframe's stamp
    std::vector<types::KfWindowPose> kf_window;  // setKeyframeWindow: the current keyframe and the members against the new map (empty: none)
    // edge-polyline callbacks: the new map's polylines, one extraction per callback, with the pose they were extracted at
    std::vector<rebvio::EdgeMap::EdgePolylines> polylines;
    types::CloudPose polyline_pose;
    // edge-segment callbacks: the same for the new map's straight segments (at polyline_pose)
    std::vector<rebvio::EdgeMap::EdgeSegments> segments;
    // depth images: a fusion into the new map was queued behind the second half; its counts (fetched where the pair's counters are)
    bool have_depth = false;
    types::DepthPriorCounts depth_counts;
    // the stereo partner: the same for the fusion of the right frame's edge map
    bool have_stereo = false;
    types::StereoPriorCounts stereo_counts;
    // setPlaceRecognition: the new map was marked and the database queried with it; the matches under max_distance
    bool have_place = false;
    std::vector<types::PlaceMatch> place_matches;
  } pending;
  // the stereo partner. take_right: the queued right image with exactly this stamp (older ones are dropped and counted); nothing is
  // touched while no right image has ever been handed in. queue_stereo: the image through the right detector, then the fusion on
  // the track stream in call order. The right map used two fusions ago is free, as the depth images' staging frames are.
  auto take_right = [&](uint64_t ts_us, types::Image* out, types::StereoPriorOpts* opts) -> bool {
    if (right_seen_.load() == 0) return false;
    std::lock_guard<std::mutex> guard(stereo_mutex_);
    while (!right_queue_.empty() && right_queue_.front().ts_us < ts_us) {
      right_queue_.pop_front();
      ++right_dropped_;
    }
    if (right_queue_.empty() || right_queue_.front().ts_us != ts_us) return false;
    *out = std::move(right_queue_.front());
    right_queue_.pop_front();
    *opts = stereo_opts_;
    return true;
  };
  auto queue_stereo = [&](rebvio::EdgeMap& map, types::Image& right, const types::StereoPriorOpts& opts) {
    rebvio::EdgeMap::SharedPtr& hold = right_hold_[right_hold_turn_++ & 1u];
    hold = right_detector_->detect(right);
    backend::check("rebvio_hip_map_fuse_stereo_async",
                   rebvio_hip_map_fuse_stereo_async(ctx, map.handle(), hold->handle(), reinterpret_cast<const rebvio_hip_stereo_prior_opts*>(&opts)));
    map.invalidateMirror();
  };
  bool have_first_stereo = false;
  uint64_t first_stereo_ts = 0;
  types::StereoPriorCounts first_stereo_counts;
  // depth images. take_depth: the queued image with exactly this stamp (older ones are dropped and counted); nothing is touched
  // while no image has ever been handed in. queue_depth: the image into one of the two device staging frames, then the fusion on
  // the track stream in call order. The frame used two fusions ago is free: a pair's first half, which the thread has waited for
  // by then, runs behind every earlier fusion.
  auto take_depth = [&](uint64_t ts_us, QueuedDepth* out, types::DepthPriorOpts* opts) -> bool {
    if (depth_seen_.load() == 0) return false;
    std::lock_guard<std::mutex> guard(depth_mutex_);
    while (!depth_queue_.empty() && depth_queue_.front().ts_us < ts_us) {
      depth_queue_.pop_front();
      ++depth_dropped_;
    }
    if (depth_queue_.empty() || depth_queue_.front().ts_us != ts_us) return false;
    *out = std::move(depth_queue_.front());
    depth_queue_.pop_front();
    *opts = depth_opts_;
    return true;
  };
  auto queue_depth = [&](rebvio::EdgeMap& map, const QueuedDepth& d, types::DepthPriorOpts opts) {
    void*& dev = depth_dev_[depth_dev_turn_++ & 1u];
    if (!dev) backend::check("rebvio_hip_device_alloc", rebvio_hip_device_alloc(ctx, (size_t)camera_.rows_ * camera_.cols_ * sizeof(float), &dev));
    backend::check("rebvio_hip_device_upload", rebvio_hip_device_upload(ctx, dev, d.bytes.data(), d.bytes.size()));
    if (d.unit > 0.0) opts.unit = d.unit;
    backend::check("rebvio_hip_map_fuse_depth_image_async",
                   rebvio_hip_map_fuse_depth_image_async(ctx, map.handle(), dev, 0, d.format, reinterpret_cast<const rebvio_hip_depth_prior_opts*>(&opts)));
    map.invalidateMirror();
  };
  bool first_pair = true;          // the stream's first map takes its image in front of the first pair
  bool have_first_depth = false;   // ... and its counts go out with the first record
  uint64_t first_depth_ts = 0;
  types::DepthPriorCounts first_depth_counts;
  // keyframe-pose callbacks: the snapshot of the current keyframe and the last pose estimated against it (the next one's guess)
  rebvio::KeyframeSnapshot kf_snapshot;
  types::KfPose kf_pose_last;
  bool kf_pose_warm = false;
  // setKeyframeWindow: the retired keyframes that are still aligned to every new map, newest first - snapshot, stamp, and the last
  // status-0 pose (the next alignment's guess; warm: there is one)
  struct KfWindowMember {
    rebvio::KeyframeSnapshot snapshot;
    uint64_t ts_us;
    types::KfPose last;
    bool warm;
  };
  std::deque<KfWindowMember> kf_window;
  // setPlaceRecognition: the signatures of the maps keyframes were marked on, made at the first mark
  rebvio::PlaceDb place_db;
  bool kf_marked_here = false;  // this pair's new map is the one the snapshot was taken from: it is not fused into itself
  // keyframe-cloud callbacks: stamp and odometry pose (R_global, Pos, K) of the record on whose map the snapshot was taken
  uint64_t kf_ts = 0;
  types::CloudPose kf_odometry_pose;
  // Two steps: the counters (and with them the stop conditions of rebvio.cpp:236-252) are fetched as soon as the next pair's
  // first half is back; the callbacks run after that pair's second half has been launched, off the path between its halves.
  auto publish_pending = [&]() {
    if (!pending.fetched) return;
    pending.fetched = false;
    for (auto& cb : odometry_callbacks_) cb(pending.odometry);
    if (have_first_depth) {
      have_first_depth = false;
      for (auto& cb : depth_prior_callbacks_) cb(first_depth_ts, first_depth_counts);
    }
    if (pending.have_depth)
      for (auto& cb : depth_prior_callbacks_) cb(pending.odometry.ts_us, pending.depth_counts);
    if (have_first_stereo) {
      have_first_stereo = false;
      for (auto& cb : stereo_prior_callbacks_) cb(first_stereo_ts, first_stereo_counts);
    }
    if (pending.have_stereo)
      for (auto& cb : stereo_prior_callbacks_) cb(pending.odometry.ts_us, pending.stereo_counts);
    if (!keyframe_callbacks_.empty()) {
      const int keylines = pending.new_map->size();
      for (auto& cb : keyframe_callbacks_) cb(pending.odometry.ts_us, pending.kf_matches, keylines);
    }
    if (pending.have_kf_pose)
      for (auto& cb : keyframe_pose_callbacks_) cb(pending.odometry.ts_us, pending.kf_pose);
    if (pending.have_kf_fuse)
      for (auto& cb : keyframe_fuse_callbacks_) cb(pending.odometry.ts_us, pending.kf_fuse);
    if (pending.have_kf_handover)
      for (auto& cb : keyframe_handover_callbacks_) cb(pending.odometry.ts_us, pending.kf_handover_ts, pending.kf_handover);
    if (!pending.kf_window.empty())
      for (auto& cb : keyframe_window_callbacks_) cb(pending.odometry.ts_us, pending.kf_window);
    // every cloud goes back to its pool, also when a callback (or the wait) throws
    struct CloudsBack {
      std::vector<rebvio_hip_cloud*>& v;
      ~CloudsBack() {
        for (rebvio_hip_cloud* cl : v) rebvio_hip_cloud_release(cl);
        v.clear();
      }
    } clouds_back{pending.clouds}, kf_clouds_back{pending.kf_clouds};
    for (size_t i = 0; i < pending.kf_clouds.size(); ++i) {  // the keyframe this record's map replaced
      const rebvio_hip_cloud_point* pts = nullptr;
      int n = 0;
      backend::check("rebvio_hip_cloud_wait", rebvio_hip_cloud_wait(pending.kf_clouds[i], &pts, &n, nullptr));  // (has run: fetch_pending)
      const types::PointCloud pc{pending.kf_cloud_ts, pending.kf_cloud_pose, reinterpret_cast<const types::CloudPoint*>(pts), (size_t)n};
      keyframe_cloud_callbacks_[i].cb(pc);
    }
    if (pending.have_place)  // after the other keyframe callbacks of the record
      for (auto& cb : place_callbacks_) cb(pending.odometry.ts_us, pending.place_matches);
    for (size_t i = 0; i < pending.clouds.size(); ++i) {
      const rebvio_hip_cloud_point* pts = nullptr;
      int n = 0;
      backend::check("rebvio_hip_cloud_wait", rebvio_hip_cloud_wait(pending.clouds[i], &pts, &n, nullptr));  // (has run: fetch_pending)
      const types::PointCloud pc{pending.odometry.ts_us, pending.cloud_pose, reinterpret_cast<const types::CloudPoint*>(pts), (size_t)n};
      point_cloud_callbacks_[i].cb(pc);
    }
    for (size_t i = 0; i < pending.polylines.size(); ++i) {
      const rebvio::EdgeMap::EdgePolylines& p = pending.polylines[i];
      const types::EdgePolylines ep{pending.odometry.ts_us, pending.polyline_pose, p.points.data(), reinterpret_cast<const int*>(p.refs.data()),
                                    p.points.size(), p.lines.data(), p.lines.size()};
      edge_polyline_callbacks_[i].cb(ep);
    }
    pending.polylines.clear();
    for (size_t i = 0; i < pending.segments.size(); ++i) {
      const rebvio::EdgeMap::EdgeSegments& g = pending.segments[i];
      const types::EdgeSegments es{pending.odometry.ts_us, pending.polyline_pose, g.segments.data(), g.segments.size(), g.counts};
      edge_segment_callbacks_[i].cb(es);
    }
    pending.segments.clear();
    pending.old_map.reset();
    pending.new_map.reset();
    ++num_published_;
  };
  auto fetch_pending = [&]() -> bool {
    if (!pending.have) return true;
    pending.have = false;
    pending.fetched = true;
    int klm_num = 0, kf_matches = 0, reg_num = 0, status = 0;
    backend::check("rebvio_hip_track_pair_result", rebvio_hip_track_pair_result(ctx, &klm_num, &kf_matches, &reg_num, &status));
    if (pending.have_depth)  // queued right behind that second half, and nothing of the kind since
      backend::check("rebvio_hip_depth_prior_last_counts",
                     rebvio_hip_depth_prior_last_counts(ctx, reinterpret_cast<rebvio_hip_depth_prior_counts*>(&pending.depth_counts)));
    if (pending.have_stereo)
      backend::check("rebvio_hip_stereo_prior_last_counts",
                     rebvio_hip_stereo_prior_last_counts(ctx, reinterpret_cast<rebvio_hip_stereo_prior_counts*>(&pending.stereo_counts)));
    for (rebvio_hip_cloud* cl : pending.clouds) {  // queued right behind that second half
      int n = 0;
      backend::check("rebvio_hip_cloud_wait", rebvio_hip_cloud_wait(cl, nullptr, &n, nullptr));
    }
    for (rebvio_hip_cloud* cl : pending.kf_clouds) {  // ... and so was a retired keyframe's
      int n = 0;
      backend::check("rebvio_hip_cloud_wait", rebvio_hip_cloud_wait(cl, nullptr, &n, nullptr));
    }
    pending.old_map->invalidateMirror();
    pending.new_map->invalidateMirror();
    bool ok = true;
    if (status == 1) {  // rebvio.cpp:236-241
      P_Kp = FMAX;
      std::cerr << "Minimization Error occured!\n";
      run_ = false;
      ok = false;
    } else if (status == 2) {  // rebvio.cpp:247-252
      P_Kp = FMAX;
      std::cerr << "Insufficient number of keylines matches!\n";
      run_ = false;
      ok = false;
    }
    pending.odometry.klm_num = klm_num;
    pending.kf_matches = kf_matches;
    return ok;
  };
  auto complete_pending = [&]() -> bool {
    const bool ok = fetch_pending();
    publish_pending();
    return ok;
  };

  while (run_) {
    rebvio::EdgeMap::SharedPtr new_edge_map, old_edge_map;
    {
      std::lock_guard<std::mutex> guard(edge_map_buffer_mutex_);
      if (edge_map_buffer_.size() >= 2) {
        old_edge_map = edge_map_buffer_.front();
        edge_map_buffer_.pop_front();
        new_edge_map = edge_map_buffer_.front();
      }
    }
    if (!new_edge_map) {
      if (pending.have) {  // nothing to overlap with: finish the last pair now
        complete_pending();
        continue;
      }
      std::this_thread::sleep_for(std::chrono::microseconds(200));
      continue;
    }

    types::Matrix3f P_V = TooN::Identity * FMAX, P_W = TooN::Identity * FMAX;

    // IMU state initialisation (rebvio.cpp:145-160)
    const rebvio::types::IntegratedImu& imu = new_edge_map->imu().get(camera_.getRc2i(), camera_.getTc2i());
    if (!imu_state_.initialized && num_frames_ > 0) {
      if (config_.imu_state.init_bias > 0) {
        gyro_init += imu.gyro() * imu.dt_s();
        g_init -= imu.cacc();
        if (++num_gyro_init > config_.imu_state.init_bias_frame_num) {
          imu_state_.Bg = gyro_init / types::Float(num_gyro_init);
          imu_state_.W_Bg = types::invert(imu_state_.RGBias * types::Float(1e2));
          const types::Vector3f g0 = g_init / types::Float(num_gyro_init);
          for (int i = 0; i < 3; ++i) sab_state_.X[1 + i] = g0[i];
          imu_state_.initialized = true;
        }
      } else {
        imu_state_.initialized = true;
        imu_state_.Bg = config_.imu_state.init_bias_guess * imu.dt_s();
      }
      if (imu_state_.initialized) {
        float bg[3] = {imu_state_.Bg[0], imu_state_.Bg[1], imu_state_.Bg[2]}, wb[9];
        store3(imu_state_.W_Bg, wb);
        rebvio_hip_set_gyro_state(ctx, bg, wb);
      }
    }

    // depth images: the stream's first map has been no pair's new map - its image goes in right behind its detection
    QueuedDepth depth_image;
    types::DepthPriorOpts depth_opts;
    types::Image right_image;
    types::StereoPriorOpts stereo_opts;
    if (first_pair) {
      first_pair = false;
      if (take_depth(old_edge_map->ts_us(), &depth_image, &depth_opts)) {
        queue_depth(*old_edge_map, depth_image, depth_opts);
        backend::check("rebvio_hip_depth_prior_last_counts",
                       rebvio_hip_depth_prior_last_counts(ctx, reinterpret_cast<rebvio_hip_depth_prior_counts*>(&first_depth_counts)));
        first_depth_ts = old_edge_map->ts_us();
        have_first_depth = true;
      }
      if (take_right(old_edge_map->ts_us(), &right_image, &stereo_opts)) {  // (behind the depth image, where there is one)
        queue_stereo(*old_edge_map, right_image, stereo_opts);
        backend::check("rebvio_hip_stereo_prior_last_counts",
                       rebvio_hip_stereo_prior_last_counts(ctx, reinterpret_cast<rebvio_hip_stereo_prior_counts*>(&first_stereo_counts)));
        first_stereo_ts = old_edge_map->ts_us();
        have_first_stereo = true;
      }
    }

    // first half on the device (rebvio.cpp:142-192)
    float Rp[9];
    store3(imu.R(), Rp);
    const types::Float frame_dt = types::Float(new_edge_map->ts_us() - old_edge_map->ts_us()) / 1000000.0;
    rebvio_hip_pair_mid mid;
    timers.start();
    backend::check("rebvio_hip_track_pair_begin",
                   rebvio_hip_track_pair_begin(ctx, old_edge_map->handle(), new_edge_map->handle(), Rp, frame_dt, &mid));
    // this pair's first half (and its parked second half) are queued behind the previous pair's second half: now that pair's
    // counters can be fetched without leaving the GPU idle
    if (!fetch_pending()) {
      publish_pending();
      const float nanv[3] = {std::numeric_limits<float>::quiet_NaN(), 0.f, 0.f}, I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
      int st = 0;  // the run has ended: let this pair's parked second half fall through
      (void)rebvio_hip_track_pair_finish(ctx, old_edge_map->handle(), new_edge_map->handle(), nanv, I9, I9, I9, nullptr, nullptr, nullptr, &st);
      break;
    }
    {
      float bg[3], wb[9];
      rebvio_hip_get_gyro_state(ctx, bg, wb);
      imu_state_.Bg = TooN::makeVector(bg[0], bg[1], bg[2]);
      imu_state_.W_Bg = load3(wb);
    }
    // the noise models the backend applied in gyroBiasCorrection (rebvio.cpp:186-187); RGBias feeds next frame's W_Bg init
    imu_state_.RGBias = TooN::Identity * (double)(config_.imu_state.gyro_bias_std_dev * config_.imu_state.gyro_bias_std_dev * frame_dt * frame_dt);
    imu_state_.RGyro = TooN::Identity * (double)(config_.imu_state.gyro_std_dev * config_.imu_state.gyro_std_dev * frame_dt * frame_dt);
    timers.lap(0);
    imu_state_.Vg = TooN::makeVector(mid.Vg[0], mid.Vg[1], mid.Vg[2]);
    imu_state_.P_Vg = load3(mid.P_Vg);
    types::Vector6f Xgv, Xgva;
    types::Matrix6f W_Xgv;
    for (int i = 0; i < 6; ++i) {
      Xgv[i] = mid.Xgv[i];
      for (int j = 0; j < 6; ++j) W_Xgv(i, j) = mid.W_Xgv[i * 6 + j];
    }
    imu_state_.dVgv = Xgv.slice<0, 3>();
    imu_state_.dWgv = Xgv.slice<3, 3>();

    // rebvio.cpp:195-203
    types::Matrix3f R = load3(mid.R);
    types::Matrix3f Rgva = R;
    const types::Matrix3f R0 = TooN::SO3<types::Float>(imu_state_.dWgv).get_matrix();
    R = (R0 * R.T()).T();
    imu_state_.Vgv = R0 * imu_state_.Vg + imu_state_.dVgv;
    {
      float A6[36], inv[36];
      for (int i = 0; i < 36; ++i) A6[i] = mid.W_Xgv[i];
      rh::hm::cholesky6_inverse(A6, inv);
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
          P_V(i, j) = inv[i * 6 + j];
          P_W(i, j) = inv[(3 + i) * 6 + 3 + j];
        }
    }

    // rebvio.cpp:206-209
    core_.estimateLs4Acceleration(-imu_state_.Vgv / frame_dt, imu_state_.Av, R, frame_dt);
    core_.estimateMeanAcceleration(imu.cacc(), imu_state_.As, R);
    Xgva = Xgv;
    sab_state_.Rv = P_V / (frame_dt * frame_dt * frame_dt * frame_dt);
    sab_state_.Qrot = P_W;
    sab_state_.QKp = P_Kp;

    types::Matrix3f R_second;
    if (num_frames_ > 4u + (unsigned)config_.imu_state.init_bias_frame_num) {  // rebvio.cpp:210-224
      const auto tb0 = timers.on ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point();
      fusion_dump.before(imu_state_.As, imu_state_.Av, 1.0, R, sab_state_, W_Xgv, Xgva, config_.imu_state.g_norm);
      K = core_.estimateBias(imu_state_.As, imu_state_.Av, 1.0, R, sab_state_.X, sab_state_.P, sab_state_.Qg, sab_state_.Qrot,
                             sab_state_.Qbias, sab_state_.QKp, sab_state_.Rg, sab_state_.Rs, sab_state_.Rv, sab_state_.g_est,
                             sab_state_.b_est, W_Xgv, Xgva, config_.imu_state.g_norm);
      if (timers.on) timers.t_bias += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tb0).count();
      fusion_dump.after(K, sab_state_, Xgva);
      imu_state_.dVgva = Xgva.slice<0, 3>();
      imu_state_.dWgva = Xgva.slice<3, 3>();
      const types::Matrix3f R0gva = TooN::SO3<types::Float>(imu_state_.dWgva).get_matrix();
      Rgva = (R0gva * Rgva.T()).T();
      imu_state_.Vgva = R0gva * imu_state_.Vg + imu_state_.dVgva;
      R_second = R0gva;
    } else {  // rebvio.cpp:225-233
      Rgva = R;
      imu_state_.Vgva = imu_state_.Vgv;
      R_second = R0;
    }

    // second half on the device (rebvio.cpp:222/232, 236-259)
    float V[3] = {imu_state_.Vgva[0], imu_state_.Vgva[1], imu_state_.Vgva[2]}, pv[9], rg[9], r2[9];
    store3(P_V, pv);
    store3(Rgva, rg);
    store3(R_second, r2);
    timers.lap(1);
    // gravity-aligned pose integration (rebvio.cpp:263-271): needs nothing from the device. With a point-cloud callback it runs
    // ahead of the hand-over, because the pair's cloud is queued with this pose right behind the second half; with a keyframe-cloud
    // callback too, which remembers this pose where a keyframe is marked.
    auto integrate_pose = [&]() {
      if (num_frames_ > 4u + (unsigned)config_.imu_state.init_bias_frame_num) {
        imu_state_.u_est = Rgva.T() * imu_state_.u_est;
        imu_state_.u_est =
            imu_state_.u_est - (imu_state_.u_est * sab_state_.g_est) / (sab_state_.g_est * sab_state_.g_est) * sab_state_.g_est;
        imu_state_.u_est = imu_state_.u_est / std::sqrt(imu_state_.u_est * imu_state_.u_est);
        const types::Matrix3f R1 = TooN::SO3<types::Float>(sab_state_.g_est, TooN::makeVector(0.0f, 1.0f, 0.0f)).get_matrix();
        const types::Matrix3f R2 = TooN::SO3<types::Float>(R1 * imu_state_.u_est, TooN::makeVector(1.0f, 0.0f, 0.0f)).get_matrix();
        R_global = R2 * R1;
        Pos += -(R_global * imu_state_.Vgva) * K;
      }
    };
    const bool want_cloud = !point_cloud_callbacks_.empty();
    const bool want_kf_pose = !keyframe_pose_callbacks_.empty();
    const bool want_kf_cloud = !keyframe_cloud_callbacks_.empty();
    const bool want_polylines = !edge_polyline_callbacks_.empty() || !edge_segment_callbacks_.empty();  // (segments: lines of the same frame)
    std::vector<rebvio_hip_cloud*> clouds, kf_clouds;
    types::CloudPose cloud_pose, kf_cloud_pose;
    uint64_t kf_cloud_ts = 0;
    if (want_cloud || want_kf_cloud || want_polylines) integrate_pose();
    // If the following frame is already queued, its gyro pre-integration (complete before the map was queued) is the next
    // pair's prior: that pair's first rotateKeylines then rides in this pair's last kernel. Only once the gyro bias is
    // initialised (until then the bias still changes between pairs, rebvio.cpp:146-160). Not with a point-cloud callback: the
    // cloud shows the new map in THIS pair's frame, so the next pair's _begin launches its rotation itself.
    // Nor with a keyframe-pose or keyframe-cloud callback: snapshot and pose take the new map in this pair's frame as well.
    // Nor while a depth image waits for the new map: it is folded into the map's depths in THIS pair's frame.
    const bool have_depth = take_depth(new_edge_map->ts_us(), &depth_image, &depth_opts);
    const bool have_stereo = take_right(new_edge_map->ts_us(), &right_image, &stereo_opts);  // (the same holds for a right image)
    // setPlaceRecognition: a keyframe request is taken here, not at the mark below - the marked map's signature is of its gradients
    // in THIS pair's frame, so the next pair's rotation must not ride in this pair's last kernel. Off, the request is read where
    // it always was.
    const int place_capacity = place_capacity_.load();
    const bool kf_taken_early = place_capacity > 0 && keyframe_requested_.exchange(false);
    float Rnext[9];
    bool have_next = false;
    rebvio::EdgeMap::SharedPtr next_map;
    {
      std::lock_guard<std::mutex> guard(edge_map_buffer_mutex_);
      if (edge_map_buffer_.size() >= 2) {
        next_map = edge_map_buffer_[1];
        if (imu_state_.initialized && !want_cloud && !want_kf_pose && !want_kf_cloud && !want_polylines && !have_depth && !have_stereo && !kf_taken_early) {
          store3(next_map->imu().R(), Rnext);
          have_next = true;
        }
      }
    }
    // the track stream's wait for the next frame's detection goes in ahead of this pair's second half
    if (next_map) backend::check("rebvio_hip_track_pair_hint_next", rebvio_hip_track_pair_hint_next(ctx, next_map->handle()));
    backend::check("rebvio_hip_track_pair_finish_async",
                   rebvio_hip_track_pair_finish_async(ctx, old_edge_map->handle(), new_edge_map->handle(), V, pv, rg, r2,
                                                      have_next ? Rnext : nullptr));
    // the depth image of the new map's frame, right behind the second half (which has written the map's depths for the last time
    // as a new map) and in front of everything that reads them: clouds, keyframe snapshots, polylines, the next pair
    if (have_depth) queue_depth(*new_edge_map, depth_image, depth_opts);
    if (have_stereo) queue_stereo(*new_edge_map, right_image, stereo_opts);  // the depth image first
    if (want_cloud) {
      store3(R_global, cloud_pose.R);
      for (int i = 0; i < 3; ++i) cloud_pose.t[i] = Pos[i];
      cloud_pose.scale = K;
      for (const PointCloudCallback& pcc : point_cloud_callbacks_) {
        rebvio_hip_cloud* cl = nullptr;
        backend::check("rebvio_hip_map_point_cloud_async",
                       rebvio_hip_map_point_cloud_async(ctx, new_edge_map->handle(), reinterpret_cast<const rebvio_hip_cloud_filter*>(&pcc.filter),
                                                        reinterpret_cast<const rebvio_hip_cloud_pose*>(&cloud_pose), &cl));
        clouds.push_back(cl);
      }
    }
    // Rebvio::requestKeyframe: the new map is marked behind this pair's second half (which writes the previous keyframe's ids into
    // it), in front of the next pair's first half (which hands the ids on)
    kf_marked_here = false;
    // setKeyframeDepthHandover: the keyframe this mark retires, where its depths are to go on to the new one - as the window's newest
    // member (handover_in_window), or kept here until its alignment behind publish_pending()
    bool handover_in_window = false;
    rebvio::KeyframeSnapshot handover_outgoing;
    types::KfPose handover_guess;
    uint64_t handover_ts = 0;
    const bool kf_mark = place_capacity > 0 ? kf_taken_early : keyframe_requested_.exchange(false);
    if (kf_mark) {
      new_edge_map->markKeyframe();
      if (want_kf_pose || want_kf_cloud) {  // the keyframe as it is now, right behind its mark; the previous one goes
        if (want_kf_cloud && kf_snapshot) {  // ... as a cloud, queued before its snapshot is released (which is safe right behind)
          kf_cloud_pose = kf_odometry_pose;
          kf_cloud_ts = kf_ts;
          for (const PointCloudCallback& pcc : keyframe_cloud_callbacks_) {
            rebvio_hip_cloud* cl = nullptr;
            backend::check("rebvio_hip_kf_snapshot_point_cloud_async",
                           rebvio_hip_kf_snapshot_point_cloud_async(kf_snapshot.handle(), reinterpret_cast<const rebvio_hip_cloud_filter*>(&pcc.filter),
                                                                    reinterpret_cast<const rebvio_hip_cloud_pose*>(&kf_cloud_pose), &cl));
            kf_clouds.push_back(cl);
          }
        }
        // setKeyframeWindow: the outgoing keyframe stays, behind its cloud; the oldest member makes room
        const int kf_window_n = (want_kf_pose && keyframe_align_) ? keyframe_window_.load() : 0;
        const bool handover = want_kf_pose && keyframe_align_ && keyframe_depth_handover_ && kf_snapshot && kf_pose_warm;
        if (handover) {
          handover_ts = kf_ts;
          handover_guess = kf_pose_last;
          handover_in_window = kf_window_n > 0;
          if (!handover_in_window) handover_outgoing = std::move(kf_snapshot);
        }
        if (kf_window_n > 0 && kf_snapshot) kf_window.push_front(KfWindowMember{std::move(kf_snapshot), kf_ts, kf_pose_last, kf_pose_warm});
        while ((int)kf_window.size() > kf_window_n) kf_window.pop_back();
        kf_snapshot = new_edge_map->keyframeSnapshot();
        kf_ts = new_edge_map->ts_us();
        store3(R_global, kf_odometry_pose.R);
        for (int i = 0; i < 3; ++i) kf_odometry_pose.t[i] = Pos[i];
        kf_odometry_pose.scale = K;
        if (keyframe_align_) kf_snapshot.addNormals(*new_edge_map);  // (setKeyframeAlign: the alignment's gradient test)
        kf_pose_warm = false;
        kf_marked_here = true;
      }
    }
    publish_pending();  // the previous pair's record: its callbacks run while the device works on this pair's second half
    // setPlaceRecognition: the marked map against the database, right behind its snapshot in stream order (the query waits for this
    // pair's second half), then the map itself goes in. The last exclude_last entries are the keyframes the tracker has just left.
    bool have_place = false;
    std::vector<types::PlaceMatch> place_matches;
    if (kf_mark && place_capacity > 0) {
      if (!place_db) place_db = new_edge_map->placeDb(place_capacity);
      const uint32_t max_distance = place_max_distance_.load();
      for (const types::PlaceMatch& m : place_db.query(*new_edge_map, place_top_k_.load(), place_exclude_last_.load()))
        if (m.distance <= max_distance) place_matches.push_back(m);
      if (place_db.add(*new_edge_map, new_edge_map->ts_us()) < 0) ++place_misses_;
      ++place_queries_;
      place_matches_ += (unsigned int)place_matches.size();
      have_place = true;
    }
    // edge-polyline callbacks: the new map's polylines in this pair's frame, behind this pair's second half (the call waits for it)
    std::vector<rebvio::EdgeMap::EdgePolylines> polylines;
    std::vector<rebvio::EdgeMap::EdgeSegments> segments;
    types::CloudPose polyline_pose;
    if (want_polylines) {
      store3(R_global, polyline_pose.R);
      for (int i = 0; i < 3; ++i) polyline_pose.t[i] = Pos[i];
      polyline_pose.scale = K;
      for (const EdgePolylineCallback& epc : edge_polyline_callbacks_) polylines.push_back(new_edge_map->edgePolylines(epc.opts, polyline_pose));
      for (const EdgeSegmentCallback& esc : edge_segment_callbacks_) segments.push_back(new_edge_map->edgeSegments(esc.opts, polyline_pose));
    }
    // keyframe-pose callbacks: the new map against the keyframe, behind this pair's second half (the call waits for it)
    bool have_kf_pose = false;
    bool have_kf_handover = false;
    types::KfHandover kf_handover;
    std::vector<types::KfWindowPose> kf_window_poses;
    if (want_kf_pose && kf_snapshot) {
      if (keyframe_align_ && keyframe_window_ > 0) {
        // the current keyframe and the window's members against the new map, in one set of launches
        std::vector<types::KfHypothesis> hyp(1 + kf_window.size());
        auto start = [](types::KfHypothesis& h, const rebvio::KeyframeSnapshot& sn, const types::KfPose* guess) {
          h.snapshot = &sn;
          if (!guess) return;
          std::memcpy(h.R0, guess->R, sizeof(h.R0));
          std::memcpy(h.t0, guess->t, sizeof(h.t0));
        };
        start(hyp[0], kf_snapshot, kf_pose_warm ? &kf_pose_last : nullptr);
        for (size_t k = 0; k < kf_window.size(); ++k) start(hyp[1 + k], kf_window[k].snapshot, kf_window[k].warm ? &kf_window[k].last : nullptr);
        const std::vector<types::KfHypResult> res = new_edge_map->keyframeAlignMany(hyp, types::KfAlignOpts());
        kf_pose_last = res[0].pose;
        kf_window_poses.push_back(types::KfWindowPose{kf_ts, res[0].pose, res[0].inliers});
        for (size_t k = 0; k < kf_window.size(); ++k) {
          kf_window_poses.push_back(types::KfWindowPose{kf_window[k].ts_us, res[1 + k].pose, res[1 + k].inliers});
          kf_window[k].last = res[1 + k].pose;
          kf_window[k].warm = res[1 + k].pose.status == 0;
        }
        // setKeyframeDepthHandover: the window's own result for its newest member is the outgoing keyframe against the new map
        if (handover_in_window && !kf_window.empty() && kf_window[0].ts_us == handover_ts && res[1].pose.status == 0) {
          kf_handover = kf_snapshot.handoverDepth(kf_window[0].snapshot, *new_edge_map, res[1].pose);
          have_kf_handover = true;
        }
        for (size_t k = kf_window.size(); k-- > 0;)  // a member that was lost leaves (reported once, above)
          if (!kf_window[k].warm) kf_window.erase(kf_window.begin() + (std::ptrdiff_t)k);
      } else if (keyframe_align_) {
        if (!kf_window.empty()) kf_window.clear();  // (the window was set to 0 with members in it)
        kf_pose_last = new_edge_map->keyframeAlign(kf_snapshot, types::KfAlignOpts(), kf_pose_warm ? &kf_pose_last : nullptr);
      } else
        kf_pose_last = new_edge_map->keyframePose(kf_snapshot, types::KfPoseOpts(), kf_pose_warm ? &kf_pose_last : nullptr);
      kf_pose_warm = kf_pose_last.status == 0;
      have_kf_pose = true;
    }
    // setKeyframeDepthHandover without a window: one alignment of the outgoing keyframe to the newly marked map, warm-started from its
    // last pose, behind the mark's own pose above (which so is what it is without the switch); then the outgoing snapshot goes
    if (handover_outgoing) {
      if (have_kf_pose && keyframe_align_) {
        const types::KfPose ho = new_edge_map->keyframeAlign(handover_outgoing, types::KfAlignOpts(), &handover_guess);
        if (ho.status == 0) {
          kf_handover = kf_snapshot.handoverDepth(handover_outgoing, *new_edge_map, ho);
          have_kf_handover = true;
        }
      }
      handover_outgoing.reset();
    }
    // setKeyframeDepthFusion: behind an alignment of status 0 the new map is one more view of the keyframe's edges from a known pose
    bool have_kf_fuse = false;
    types::KfFuse kf_fuse;
    if (have_kf_pose && keyframe_align_ && keyframe_depth_fusion_ && !kf_marked_here && kf_pose_last.status == 0) {
      kf_fuse = kf_snapshot.fuseDepth(*new_edge_map, kf_pose_last);
      have_kf_fuse = true;
    }
    timers.lap(2);

    if (!want_cloud && !want_kf_cloud && !want_polylines) integrate_pose();
    types::Odometry odometry;
    odometry.ts_us = new_edge_map->ts_us();
    odometry.orientation = TooN::SO3<types::Float>(R_global).ln();
    odometry.position = Pos;
    odometry.scale = K;
    odometry.gravity = sab_state_.g_est;
    odometry.gyro_bias = imu_state_.Bg;
    pending.have = true;  // published by complete_pending() once the match count is in
    pending.odometry = odometry;
    pending.old_map = old_edge_map;
    pending.new_map = new_edge_map;
    pending.cloud_pose = cloud_pose;
    pending.clouds = clouds;
    pending.kf_clouds = kf_clouds;
    pending.kf_cloud_pose = kf_cloud_pose;
    pending.kf_cloud_ts = kf_cloud_ts;
    pending.have_kf_pose = have_kf_pose;
    pending.kf_pose = kf_pose_last;
    pending.have_kf_fuse = have_kf_fuse;
    pending.kf_fuse = kf_fuse;
    pending.have_kf_handover = have_kf_handover;
    pending.kf_handover = kf_handover;
    pending.kf_handover_ts = handover_ts;
    pending.kf_window = std::move(kf_window_poses);
    pending.polylines = std::move(polylines);
    pending.polyline_pose = polyline_pose;
    pending.segments = std::move(segments);
    pending.have_depth = have_depth;
    pending.have_stereo = have_stereo;
    pending.have_place = have_place;
    pending.place_matches = std::move(place_matches);
    timers.lap(3);
    timers.end_pair();
    timers.n++;
    ++num_frames_;
  }
  complete_pending();
}

}  // namespace rebvio
