// rebvio::Rebvio's keyframe-pose callback and EdgeMap::keyframeSnapshot / keyframePose on a synthetic stream (GPU).
//   test_keyframe_pose <frames.u8> <W> <H> <N> <fm> <cx> <cy> <keylines_ref> <keylines_max> <imu.bin> <min matches> <request at frame>
// Runs the stream three times:
//   plain    no pose callback; the pipeline is drained in front of frame R (waitIdle) and a keyframe is requested there
//   posed    the same with a pose callback: the odometry lines are byte-identical to plain; one pose per odometry record from the
//            keyframe's own record on (stamp R * 50000), none in front of it, each right after its odometry record; the first is the
//            identity within 1e-9 (the keyframe against its own snapshot) with every candidate a keyline of the keyframe; every pose
//            has status 0, finite values, an orthonormal R and 0 < used <= candidates; the translation grows away from the keyframe
//   again    posed once more: the poses are the same in every byte (nothing in the estimate depends on timing)
// and checks EdgeMap::keyframeSnapshot / keyframePose on two detected maps matched through the stepwise calls against
// EdgeMap::keyframeMatches and against what the callback reports for a keyframe: candidates, the identity for the keyframe itself, a
// warm start that stays where it is, an empty snapshot handle refused.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "rebvio/core.hpp"
#include "rebvio/edge_detector.hpp"
#include "rebvio/io/stream_io.hpp"
#include "rebvio/rebvio.hpp"

static int fails = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                \
    }                                                         \
  } while (0)

struct Args {
  std::string frames, imu;
  int W, H, N, kref, kmax, min_matches, request_at;
  float fm, cx, cy;
};

struct PoseRec {
  uint64_t ts;
  rebvio::types::KfPose pose;
  size_t odometry_seen;  // odometry records published when the call arrived
};

static bool run(const Args& a, bool with_callback, std::vector<std::string>* lines, std::vector<uint64_t>* odo_ts, std::vector<PoseRec>* recs) {
  rebvio::RebvioConfig config;
  config.camera = rebvio::Camera(a.H, a.W, a.fm, a.fm, a.cx, a.cy);
  config.edge_detector.keylines_ref = a.kref;
  config.edge_detector.keylines_max = a.kmax;
  config.core.global_min_matches_threshold = (unsigned)a.min_matches;
  rebvio::io::RawReader src(a.frames, a.H, a.W, 0, 50000, a.imu);
  rebvio::Rebvio rebvio(config);
  std::mutex mu;
  rebvio.registerOdometryCallback([&](rebvio::types::Odometry& o) {
    std::lock_guard<std::mutex> g(mu);
    lines->push_back(rebvio::io::OdometryWriter::format(o));
    odo_ts->push_back(o.ts_us);
  });
  if (with_callback)
    rebvio.registerKeyframePoseCallback([&](uint64_t ts_us, const rebvio::types::KfPose& p) {
      std::lock_guard<std::mutex> g(mu);
      recs->push_back(PoseRec{ts_us, p, odo_ts->size()});
    });
  int fed = 0;
  rebvio::io::replay(src,
                     [&](rebvio::types::Image&& im) {
                       if (fed++ == a.request_at) {
                         rebvio.waitIdle();  // every pair in front of this frame has been tracked and published
                         rebvio.requestKeyframe();
                       }
                       rebvio.imageCallback(std::move(im));
                     },
                     [&](rebvio::types::Imu&& s) { rebvio.imuCallback(std::move(s)); });
  rebvio.waitIdle();
  return rebvio.running();
}

static bool finite_pose(const rebvio::types::KfPose& p) {
  double v[55];  // R, t, H, g, cost: 55 doubles in a row
  std::memcpy(v, &p, sizeof(v));
  for (int i = 0; i < 55; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

static double from_identity(const rebvio::types::KfPose& p) {
  double d = 0;
  for (int i = 0; i < 9; ++i) d = std::fmax(d, std::fabs(p.R[i] - (i % 4 == 0 ? 1.0 : 0.0)));
  for (int i = 0; i < 3; ++i) d = std::fmax(d, std::fabs(p.t[i]));
  return d;
}

static double from_orthonormal(const rebvio::types::KfPose& p) {
  double d = 0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0;
      for (int k = 0; k < 3; ++k) s += p.R[3 * i + k] * p.R[3 * j + k];
      d = std::fmax(d, std::fabs(s - (i == j ? 1.0 : 0.0)));
    }
  return d;
}

int main(int argc, char** argv) {
  if (argc < 13) return 2;
  Args a;
  a.frames = argv[1];
  a.W = std::atoi(argv[2]); a.H = std::atoi(argv[3]); a.N = std::atoi(argv[4]);
  a.fm = (float)std::atof(argv[5]); a.cx = (float)std::atof(argv[6]); a.cy = (float)std::atof(argv[7]);
  a.kref = std::atoi(argv[8]); a.kmax = std::atoi(argv[9]);
  a.imu = argv[10];
  a.min_matches = std::atoi(argv[11]);
  a.request_at = std::atoi(argv[12]);
  try {
    std::vector<std::string> plain, with, twice;
    std::vector<uint64_t> ts_plain, ts_with, ts_twice;
    std::vector<PoseRec> none, poses, again;
    CHECK(run(a, false, &plain, &ts_plain, &none));
    CHECK(run(a, true, &with, &ts_with, &poses));
    CHECK(run(a, true, &twice, &ts_twice, &again));
    CHECK((int)plain.size() == a.N - 1 && none.empty());
    CHECK(plain == with && plain == twice);  // byte-identical odometry lines
    const uint64_t ts_kf = (uint64_t)a.request_at * 50000ull;
    CHECK(poses.size() == (size_t)(a.N - a.request_at));  // the keyframe's own record and every record behind it
    double t_prev = -1.0;
    for (size_t i = 0; i < poses.size(); ++i) {
      const PoseRec& r = poses[i];
      const size_t rec = (size_t)a.request_at - 1 + i;  // index of its odometry record
      CHECK(r.ts == ts_kf + i * 50000ull);
      CHECK(rec < ts_with.size() && ts_with[rec] == r.ts && r.odometry_seen == rec + 1);  // right after its record, before the next
      CHECK(r.pose.status == 0 && r.pose.iterations == 8);
      CHECK(finite_pose(r.pose) && from_orthonormal(r.pose) < 1e-12);
      CHECK(r.pose.used >= 12 && r.pose.used <= r.pose.candidates && r.pose.candidates <= a.kmax);
      const double tn = std::sqrt(r.pose.t[0] * r.pose.t[0] + r.pose.t[1] * r.pose.t[1] + r.pose.t[2] * r.pose.t[2]);
      std::printf("ts %llu candidates %d used %d |t| %.5f cost %.2f\n", (unsigned long long)r.ts, r.pose.candidates, r.pose.used, tn, r.pose.cost);
      if (i == 0) {
        CHECK(from_identity(r.pose) <= 1e-9 && r.pose.cost == 0.0);
        CHECK(r.pose.candidates > 100);  // every keyline of the keyframe is its own correspondence
      } else if (i <= 4) {
        CHECK(tn > t_prev);  // the camera of the synthetic stream moves steadily away from the keyframe
      }
      t_prev = tn;
    }
    CHECK(again.size() == poses.size());
    for (size_t i = 0; i < poses.size() && i < again.size(); ++i)
      CHECK(again[i].ts == poses[i].ts && std::memcmp(&again[i].pose, &poses[i].pose, sizeof(rebvio::types::KfPose)) == 0);

    // EdgeMap::keyframeSnapshot / keyframePose: frame 0 becomes the keyframe and is matched forward into frame 1 by the stepwise
    // calls. Fresh maps carry no depth yet (matches 0, the initial sigma_rho): the filter is opened for them.
    {
      auto cam = std::make_shared<rebvio::Camera>(a.H, a.W, a.fm, a.fm, a.cx, a.cy);
      auto dcfg = std::make_shared<rebvio::EdgeDetectorConfig>();
      dcfg->keylines_ref = a.kref;
      dcfg->keylines_max = a.kmax;
      rebvio::EdgeDetector detector(cam, dcfg);
      rebvio::Core core(cam);
      rebvio::io::RawReader src(a.frames, a.H, a.W, 0, 50000);
      rebvio::EdgeMap::SharedPtr maps[2];
      for (int i = 0; i < 2; ++i) {
        rebvio::types::Image img{(uint64_t)i * 50000ull, cv::Mat()};
        src.frame((size_t)i).convertTo(img.data, CV_32FC1, 3.0);
        maps[i] = detector.detect(img);
      }
      const int n0 = maps[0]->size();
      CHECK(n0 > 100);
      rebvio::types::KfPoseOpts open;
      open.kf_filter.min_matches = 0;
      open.kf_filter.max_rel_sigma = 1e9f;
      maps[0]->markKeyframe();
      rebvio::KeyframeSnapshot snap = maps[0]->keyframeSnapshot();
      CHECK((bool)snap);
      // the keyframe against itself: what the callback reports at the keyframe's record
      const rebvio::types::KfPose self = maps[0]->keyframePose(snap, open);
      CHECK(self.status == 0 && self.candidates == n0 && self.used == n0 && from_identity(self) <= 1e-9 && self.cost == 0.0);
      CHECK(maps[0]->keyframePose(snap).status == 3);  // the default filter: nothing has a depth yet
      core.buildDistanceField(maps[1]);
      rebvio::types::Vector3f vel = TooN::Zeros;
      rebvio::types::Matrix3f Rvel;
      core.minimizeVel(maps[0], vel, Rvel);
      maps[0]->forwardMatch(maps[1]);
      const size_t n_match = maps[1]->keyframeMatches(n0).size();
      const rebvio::types::KfPose p = maps[1]->keyframePose(snap, open);
      std::printf("stepwise: %zu correspondences, used %d, status %d, cost %.2f\n", n_match, p.used, p.status, p.cost);
      CHECK(n_match > 50 && p.candidates == (int)n_match && p.used > 12 && p.used <= p.candidates);
      CHECK(p.status == 0 && p.iterations == 8 && finite_pose(p) && from_orthonormal(p) < 1e-12);
      // a warm start from the result: the sums at the guess are the result's, and eight more steps stay within 1e-3 of it
      rebvio::types::KfPoseOpts eval = open;
      eval.max_iter = 0;
      const rebvio::types::KfPose at = maps[1]->keyframePose(snap, eval, &p);
      CHECK(at.iterations == 0 && std::memcmp(&at, &p, 55 * sizeof(double)) == 0 && at.used == p.used);
      const rebvio::types::KfPose warm = maps[1]->keyframePose(snap, open, &p);
      double d = 0;
      for (int i = 0; i < 9; ++i) d = std::fmax(d, std::fabs(warm.R[i] - p.R[i]));
      for (int i = 0; i < 3; ++i) d = std::fmax(d, std::fabs(warm.t[i] - p.t[i]));
      std::printf("warm start: moved by %.3g\n", d);
      CHECK(warm.status == 0 && d <= 1e-3);
      rebvio::KeyframeSnapshot moved = std::move(snap);
      CHECK(!snap && (bool)moved);
      bool refused = false;
      try {
        maps[1]->keyframePose(snap, open);  // an empty handle
      } catch (const std::exception&) {
        refused = true;
      }
      CHECK(refused);
      moved.reset();
      CHECK(!moved);
    }
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    ++fails;
  }
  if (fails == 0) std::printf("ok\n");
  return fails ? 1 : 0;
}
