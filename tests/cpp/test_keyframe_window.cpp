// rebvio::Rebvio::setKeyframeWindow / registerKeyframeWindowCallback and EdgeMap::keyframeAlignMany, keyframeAlignBest,
// keyframeHypothesesAround on a synthetic stream (GPU).
//   test_keyframe_window <frames.u8> <W> <H> <N> <fm> <cx> <cy> <keylines_ref> <keylines_max> <imu.bin> <min matches> <keyframe every>
// A keyframe is requested before the first frame and after every <keyframe every>-th odometry record, with setKeyframeAlign on and a
// keyframe-pose callback registered. Four runs:
//   none     window 0, no window callback
//   three    window 3, a window callback
//   again    the same once more
//   silent   window 3, no window callback registered
// The odometry lines and the keyframe-pose callback's (stamp, pose) records of all four are byte-identical. Every window callback of
// `three` comes right after the pose callback of its record, has the current keyframe first - its pose the pose callback's, byte
// for byte - then at most 3 members, newest first, each older than the entry before it; a member that reports a status other than 0
// is never seen again; some callback has a member. `three` and `again` are equal in every byte.
// Then EdgeMap::keyframeAlignMany on two detected maps: the pose of every hypothesis is keyframeAlign's, byte for byte; the 13 starts
// of keyframeHypothesesAround; keyframeAlignBest on the results; an empty list and an empty snapshot handle are refused.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <set>
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
  int W, H, N, kref, kmax, min_matches, every;
  float fm, cx, cy;
};

struct PoseRec {
  uint64_t ts;
  rebvio::types::KfPose pose;
};

struct WindowRec {
  uint64_t ts;
  std::vector<rebvio::types::KfWindowPose> entries;
  size_t poses_seen;  // pose callbacks that had arrived when this one did
};

struct Run {
  std::vector<std::string> lines;
  std::vector<PoseRec> poses;
  std::vector<WindowRec> windows;
  bool running = false;
};

static Run run(const Args& a, int window, bool with_window_callback) {
  Run out;
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
    out.lines.push_back(rebvio::io::OdometryWriter::format(o));
    if (out.lines.size() % (size_t)a.every == 0) rebvio.requestKeyframe();
  });
  rebvio.registerKeyframePoseCallback([&](uint64_t ts_us, const rebvio::types::KfPose& p) {
    std::lock_guard<std::mutex> g(mu);
    out.poses.push_back(PoseRec{ts_us, p});
  });
  if (with_window_callback)
    rebvio.registerKeyframeWindowCallback([&](uint64_t ts_us, const std::vector<rebvio::types::KfWindowPose>& w) {
      std::lock_guard<std::mutex> g(mu);
      out.windows.push_back(WindowRec{ts_us, w, out.poses.size()});
    });
  rebvio.setKeyframeAlign(true);
  rebvio.setKeyframeWindow(window);
  rebvio.requestKeyframe();
  // frame by frame: which record a requestKeyframe from the odometry callback lands on is then the same in every run
  rebvio::io::replay(src,
                     [&](rebvio::types::Image&& im) {
                       rebvio.waitIdle();
                       rebvio.imageCallback(std::move(im));
                     },
                     [&](rebvio::types::Imu&& s) { rebvio.imuCallback(std::move(s)); });
  rebvio.waitIdle();
  out.running = rebvio.running();
  return out;
}

static bool same_poses(const Run& x, const Run& y) {
  if (x.poses.size() != y.poses.size()) return false;
  for (size_t i = 0; i < x.poses.size(); ++i)
    if (x.poses[i].ts != y.poses[i].ts || std::memcmp(&x.poses[i].pose, &y.poses[i].pose, sizeof(rebvio::types::KfPose)) != 0) return false;
  return true;
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
  a.every = std::atoi(argv[12]);
  try {
    const Run none = run(a, 0, false), three = run(a, 3, true), again = run(a, 3, true), silent = run(a, 3, false);
    CHECK(none.running && three.running && again.running && silent.running);
    CHECK((int)none.lines.size() == a.N - 1 && !none.poses.empty());
    CHECK(none.lines == three.lines && none.lines == again.lines && none.lines == silent.lines);
    CHECK(same_poses(none, three) && same_poses(none, again) && same_poses(none, silent));
    CHECK(none.windows.empty() && silent.windows.empty());
    CHECK(three.windows.size() == three.poses.size());  // one per record that has a pose
    std::set<uint64_t> lost;
    size_t most = 0;
    uint64_t current = 0;
    std::set<uint64_t> keyframes;
    for (size_t i = 0; i < three.windows.size(); ++i) {
      const WindowRec& w = three.windows[i];
      CHECK(w.poses_seen == i + 1 && i < three.poses.size() && three.poses[i].ts == w.ts);  // right behind its record's pose callback
      CHECK(!w.entries.empty() && w.entries.size() <= 4);
      if (w.entries.empty() || i >= three.poses.size()) continue;
      most = w.entries.size() > most ? w.entries.size() : most;
      // the current keyframe first, with the pose the pose callback got
      CHECK(std::memcmp(&w.entries[0].pose, &three.poses[i].pose, sizeof(rebvio::types::KfPose)) == 0);
      CHECK(w.entries[0].kf_ts_us <= w.ts && w.entries[0].kf_ts_us >= current);
      current = w.entries[0].kf_ts_us;
      keyframes.insert(current);
      std::printf("ts %llu:", (unsigned long long)w.ts);
      for (size_t k = 0; k < w.entries.size(); ++k) {
        const rebvio::types::KfWindowPose& e = w.entries[k];
        std::printf("  kf %llu status %d used %d inliers %d", (unsigned long long)e.kf_ts_us, e.pose.status, e.pose.used, e.inliers);
        CHECK(e.inliers >= 0 && e.inliers <= e.pose.used && e.pose.used <= e.pose.candidates);
        if (k == 0) continue;
        CHECK(e.kf_ts_us < w.entries[k - 1].kf_ts_us);       // members newest first, all older than the current keyframe
        CHECK(keyframes.count(e.kf_ts_us) == 1);               // ... and each was the current keyframe once
        CHECK(lost.count(e.kf_ts_us) == 0);                    // no member reports a status other than 0 twice: it has left
        if (e.pose.status != 0) lost.insert(e.kf_ts_us);
      }
      std::printf("\n");
    }
    CHECK(keyframes.size() >= 4 && most >= 2 && most <= 4);  // keyframes were retired and at least one stayed aligned as a member
    CHECK(again.windows.size() == three.windows.size());
    for (size_t i = 0; i < three.windows.size() && i < again.windows.size(); ++i) {
      const WindowRec &x = three.windows[i], &y = again.windows[i];
      CHECK(x.ts == y.ts && x.entries.size() == y.entries.size());
      for (size_t k = 0; k < x.entries.size() && k < y.entries.size(); ++k)
        CHECK(x.entries[k].kf_ts_us == y.entries[k].kf_ts_us && x.entries[k].inliers == y.entries[k].inliers &&
              std::memcmp(&x.entries[k].pose, &y.entries[k].pose, sizeof(rebvio::types::KfPose)) == 0);
    }

    // EdgeMap::keyframeAlignMany and the two free functions on two detected maps. Fresh maps carry no depth yet (matches 0, the
    // initial sigma_rho): the filter is opened for them.
    {
      auto cam = std::make_shared<rebvio::Camera>(a.H, a.W, a.fm, a.fm, a.cx, a.cy);
      auto dcfg = std::make_shared<rebvio::EdgeDetectorConfig>();
      dcfg->keylines_ref = a.kref;
      dcfg->keylines_max = a.kmax;
      rebvio::EdgeDetector detector(cam, dcfg);
      rebvio::io::RawReader src(a.frames, a.H, a.W, 0, 50000);
      rebvio::EdgeMap::SharedPtr maps[3];
      for (int i = 0; i < 3; ++i) {
        rebvio::types::Image img{(uint64_t)i * 50000ull, cv::Mat()};
        src.frame((size_t)i).convertTo(img.data, CV_32FC1, 3.0);
        maps[i] = detector.detect(img);
      }
      rebvio::types::KfAlignOpts open;
      open.kf_filter.min_matches = 0;
      open.kf_filter.max_rel_sigma = 1e9f;
      rebvio::KeyframeSnapshot s0 = maps[0]->keyframeSnapshot(), s1 = maps[1]->keyframeSnapshot();
      s0.addNormals(*maps[0]);
      const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, z[3] = {0, 0, 0};
      std::vector<rebvio::types::KfHypothesis> hyp = rebvio::keyframeHypothesesAround(s0, I, z, 0.002, 0.005);
      CHECK(hyp.size() == 13 && hyp[0].snapshot == &s0 && std::memcmp(hyp[0].R0, I, sizeof(I)) == 0 && hyp[7].t0[0] == 0.005 && hyp[8].t0[0] == -0.005);
      rebvio::types::KfHypothesis other;  // the identity, a snapshot without normals
      other.snapshot = &s1;
      hyp.push_back(other);
      const std::vector<rebvio::types::KfHypResult> res = maps[2]->keyframeAlignMany(hyp, open);
      CHECK(res.size() == 14);
      for (size_t h = 0; h < res.size() && h < hyp.size(); ++h) {
        rebvio::types::KfPose guess;
        std::memcpy(guess.R, hyp[h].R0, sizeof(guess.R));
        std::memcpy(guess.t, hyp[h].t0, sizeof(guess.t));
        const rebvio::types::KfPose one = maps[2]->keyframeAlign(*hyp[h].snapshot, open, &guess);
        CHECK(std::memcmp(&one, &res[h].pose, sizeof(one)) == 0);
        CHECK(res[h].inliers >= 0 && res[h].inliers <= res[h].pose.used && res[h].reserved == 0);
      }
      const int best = rebvio::keyframeAlignBest(res, 12);
      std::printf("two maps: best %d", best);
      if (best >= 0) std::printf(" status %d used %d inliers %d", res[(size_t)best].pose.status, res[(size_t)best].pose.used, res[(size_t)best].inliers);
      std::printf("\n");
      CHECK(best >= 0 && best < 14 && res[(size_t)best].pose.status == 0);
      for (const rebvio::types::KfHypResult& r : res) CHECK(r.pose.status != 0 || r.inliers <= res[(size_t)best].inliers);
      CHECK(rebvio::keyframeAlignBest(res, 1 << 30) == -1);
      bool refused = false;
      try {
        maps[2]->keyframeAlignMany({}, open);
      } catch (const std::exception&) {
        refused = true;
      }
      CHECK(refused);
      refused = false;
      try {
        rebvio::keyframeAlignBest({}, 0);
      } catch (const std::exception&) {
        refused = true;
      }
      CHECK(refused);
      rebvio::KeyframeSnapshot empty;
      other.snapshot = &empty;
      refused = false;
      try {
        maps[2]->keyframeAlignMany({hyp[0], other}, open);
      } catch (const std::exception&) {
        refused = true;
      }
      CHECK(refused);
    }
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    ++fails;
  }
  if (fails == 0) std::printf("ok\n");
  return fails ? 1 : 0;
}
