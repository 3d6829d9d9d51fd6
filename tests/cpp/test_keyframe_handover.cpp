// rebvio::Rebvio::setKeyframeDepthHandover / registerKeyframeHandoverCallback and KeyframeSnapshot::handoverDepth on a synthetic stream
// (GPU).
//   test_keyframe_handover <frames.u8> <W> <H> <N> <fm> <cx> <cy> <keylines_ref> <keylines_max> <imu.bin> <min matches> <request at> <again at>
// Runs the stream eight times, the pipeline drained in front of frames R and R2 (waitIdle) and a keyframe requested at each:
//   plain    no callback at all
//   off      pose and handover callbacks, setKeyframeAlign on, the switch off
//   on       the same with setKeyframeDepthHandover on
//   again    on once more
//   noalign  pose and handover callbacks, the switch on, setKeyframeAlign off
//   nopose   a handover callback only, both switches on
//   win_off  off with setKeyframeWindow(3) and a window callback
//   win_on   on with them
// The odometry lines of all eight are byte-identical. on hands out exactly one hand-over record per mark that retires a keyframe whose
// last pose had status 0 - none at the first mark - right behind the pose record of the mark's own pair, with the retired keyframe's
// stamp, candidates = its size and claimed = adopted + kept + conflicts; every pose record up to and including that pair's is
// byte-identical to off's; again equals on in every byte; off, noalign and nopose hand out none. The same holds with the window, whose
// callbacks up to and including that record are unchanged by the switch.
// Then KeyframeSnapshot::handoverDepth on two detected maps: the counts against the association vector, the stand-in max_dist -1 for
// the context's value, src untouched, refusals.
#include <climits>
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
  int W, H, N, kref, kmax, min_matches, request_at, again_at;
  float fm, cx, cy;
};

struct PoseRec {
  uint64_t ts;
  rebvio::types::KfPose pose;
  size_t seq;  // position among all pose, window and handover calls of the run
};
struct HandoverRec {
  uint64_t ts, kf_ts;
  rebvio::types::KfHandover h;
  size_t seq;
};
struct WindowRec {
  uint64_t ts;
  std::vector<rebvio::types::KfWindowPose> w;
};

struct Run {
  std::vector<std::string> lines;
  std::vector<PoseRec> poses;
  std::vector<HandoverRec> handovers;
  std::vector<WindowRec> windows;
  bool running = false;
};

static Run run(const Args& a, bool pose_cb, bool handover_cb, bool align, bool handover, int window) {
  Run out;
  rebvio::RebvioConfig config;
  config.camera = rebvio::Camera(a.H, a.W, a.fm, a.fm, a.cx, a.cy);
  config.edge_detector.keylines_ref = a.kref;
  config.edge_detector.keylines_max = a.kmax;
  config.core.global_min_matches_threshold = (unsigned)a.min_matches;
  rebvio::io::RawReader src(a.frames, a.H, a.W, 0, 50000, a.imu);
  rebvio::Rebvio rebvio(config);
  std::mutex mu;
  size_t seq = 0;
  rebvio.registerOdometryCallback([&](rebvio::types::Odometry& o) {
    std::lock_guard<std::mutex> g(mu);
    out.lines.push_back(rebvio::io::OdometryWriter::format(o));
  });
  if (pose_cb)
    rebvio.registerKeyframePoseCallback([&](uint64_t ts_us, const rebvio::types::KfPose& p) {
      std::lock_guard<std::mutex> g(mu);
      out.poses.push_back(PoseRec{ts_us, p, seq++});
    });
  if (handover_cb)
    rebvio.registerKeyframeHandoverCallback([&](uint64_t ts_us, uint64_t kf_ts_us, const rebvio::types::KfHandover& h) {
      std::lock_guard<std::mutex> g(mu);
      out.handovers.push_back(HandoverRec{ts_us, kf_ts_us, h, seq++});
    });
  if (window > 0) {
    rebvio.registerKeyframeWindowCallback([&](uint64_t ts_us, const std::vector<rebvio::types::KfWindowPose>& w) {
      std::lock_guard<std::mutex> g(mu);
      out.windows.push_back(WindowRec{ts_us, w});
      ++seq;
    });
    rebvio.setKeyframeWindow(window);
  }
  rebvio.setKeyframeAlign(align);
  rebvio.setKeyframeDepthHandover(handover);
  int fed = 0;
  rebvio::io::replay(src,
                     [&](rebvio::types::Image&& im) {
                       if (fed == a.request_at || fed == a.again_at) {
                         rebvio.waitIdle();  // every pair in front of this frame has been tracked and published
                         rebvio.requestKeyframe();
                       }
                       ++fed;
                       rebvio.imageCallback(std::move(im));
                     },
                     [&](rebvio::types::Imu&& s) { rebvio.imuCallback(std::move(s)); });
  rebvio.waitIdle();
  out.running = rebvio.running();
  return out;
}

static bool same_pose(const rebvio::types::KfPose& x, const rebvio::types::KfPose& y) { return std::memcmp(&x, &y, sizeof(x)) == 0; }

// what one run with the switch on must show against the same run with it off
static void check_pair(const char* what, const Args& a, const Run& on, const Run& off) {
  const uint64_t ts_kf[2] = {(uint64_t)a.request_at * 50000ull, (uint64_t)a.again_at * 50000ull};
  CHECK(off.handovers.empty());
  CHECK(on.poses.size() == (size_t)(a.N - a.request_at) && off.poses.size() == on.poses.size());
  // the keyframe the second mark retires: its last pose is the record in front of the second mark's own
  int last_status = -1, kf_size = -1;
  const PoseRec* own = nullptr;
  for (size_t i = 0; i < on.poses.size(); ++i) {
    if (on.poses[i].ts == ts_kf[0]) kf_size = on.poses[i].pose.candidates;  // (the alignment's candidates = the snapshot's size)
    if (on.poses[i].ts == ts_kf[1]) {
      own = &on.poses[i];
      if (i > 0) last_status = on.poses[i - 1].pose.status;
    }
  }
  CHECK(own != nullptr && kf_size > 0);
  std::printf("%s: the retired keyframe's last status %d, size %d; hand-over records %zu\n", what, last_status, kf_size, on.handovers.size());
  CHECK(last_status == 0);  // (the stream is chosen so: the case under test)
  CHECK(on.handovers.size() == 1);
  for (const HandoverRec& r : on.handovers) {
    const rebvio::types::KfHandover& h = r.h;
    std::printf("   ts %llu kf %llu: candidates %d associated %d out_of_range %d claimed %d adopted %d kept %d conflicts %d\n",
                (unsigned long long)r.ts, (unsigned long long)r.kf_ts, h.candidates, h.associated, h.out_of_range, h.claimed, h.adopted, h.kept,
                h.conflicts);
    CHECK(r.ts == ts_kf[1] && r.kf_ts == ts_kf[0]);  // none at the first mark: it retires nothing
    CHECK(own && r.seq == own->seq + 1);  // right behind the pose record of the mark's own pair
    CHECK(h.candidates == kf_size && h.associated <= h.candidates && h.claimed == h.adopted + h.kept + h.conflicts);
    CHECK(h.out_of_range >= 0 && h.adopted >= 0 && h.kept >= 0 && h.conflicts >= 0 && h.associated - h.out_of_range - h.claimed >= 0);
    CHECK(h.associated > 12 && h.claimed > 12);
  }
  // every pose record up to and including the mark's own pair is what it is without the switch
  for (size_t i = 0; i < on.poses.size() && i < off.poses.size(); ++i) {
    CHECK(on.poses[i].ts == off.poses[i].ts);
    if (on.poses[i].ts <= ts_kf[1]) CHECK(same_pose(on.poses[i].pose, off.poses[i].pose));
  }
  // ... and so is every window record
  CHECK(on.windows.size() == off.windows.size());
  for (size_t i = 0; i < on.windows.size() && i < off.windows.size(); ++i) {
    CHECK(on.windows[i].ts == off.windows[i].ts && on.windows[i].w.size() == off.windows[i].w.size());
    if (on.windows[i].ts > ts_kf[1] || on.windows[i].w.size() != off.windows[i].w.size()) continue;
    for (size_t k = 0; k < on.windows[i].w.size(); ++k)
      CHECK(on.windows[i].w[k].kf_ts_us == off.windows[i].w[k].kf_ts_us && on.windows[i].w[k].inliers == off.windows[i].w[k].inliers &&
            same_pose(on.windows[i].w[k].pose, off.windows[i].w[k].pose));
  }
}

static void check_equal(const Run& x, const Run& y) {
  CHECK(x.poses.size() == y.poses.size() && x.handovers.size() == y.handovers.size() && x.windows.size() == y.windows.size());
  for (size_t i = 0; i < x.poses.size() && i < y.poses.size(); ++i)
    CHECK(x.poses[i].ts == y.poses[i].ts && x.poses[i].seq == y.poses[i].seq && same_pose(x.poses[i].pose, y.poses[i].pose));
  for (size_t i = 0; i < x.handovers.size() && i < y.handovers.size(); ++i)
    CHECK(x.handovers[i].ts == y.handovers[i].ts && x.handovers[i].kf_ts == y.handovers[i].kf_ts && x.handovers[i].seq == y.handovers[i].seq &&
          std::memcmp(&x.handovers[i].h, &y.handovers[i].h, sizeof(rebvio::types::KfHandover)) == 0);
}

int main(int argc, char** argv) {
  if (argc < 14) return 2;
  Args a;
  a.frames = argv[1];
  a.W = std::atoi(argv[2]); a.H = std::atoi(argv[3]); a.N = std::atoi(argv[4]);
  a.fm = (float)std::atof(argv[5]); a.cx = (float)std::atof(argv[6]); a.cy = (float)std::atof(argv[7]);
  a.kref = std::atoi(argv[8]); a.kmax = std::atoi(argv[9]);
  a.imu = argv[10];
  a.min_matches = std::atoi(argv[11]);
  a.request_at = std::atoi(argv[12]);
  a.again_at = std::atoi(argv[13]);
  try {
    const Run plain = run(a, false, false, false, false, 0), off = run(a, true, true, true, false, 0), on = run(a, true, true, true, true, 0),
              again = run(a, true, true, true, true, 0), noalign = run(a, true, true, false, true, 0), nopose = run(a, false, true, true, true, 0),
              win_off = run(a, true, true, true, false, 3), win_on = run(a, true, true, true, true, 3);
    for (const Run* r : {&plain, &off, &on, &again, &noalign, &nopose, &win_off, &win_on}) {
      CHECK(r->running);
      CHECK(r->lines == plain.lines);
    }
    CHECK((int)plain.lines.size() == a.N - 1);
    CHECK(noalign.handovers.empty() && nopose.handovers.empty() && nopose.poses.empty());
    CHECK(noalign.poses.size() == on.poses.size());
    check_pair("no window", a, on, off);
    check_equal(on, again);
    check_pair("window 3", a, win_on, win_off);
    CHECK(!win_on.windows.empty());
    // the record of the mark's own pair is the same with and without the window (the alignment of many equals the alignment of one)
    for (size_t i = 0; i < on.poses.size() && i < win_on.poses.size(); ++i)
      if (on.poses[i].ts <= (uint64_t)a.again_at * 50000ull) CHECK(same_pose(on.poses[i].pose, win_on.poses[i].pose));

    // KeyframeSnapshot::handoverDepth on two detected maps. Fresh maps carry no depth yet (matches 0, the initial rho and sigma_rho):
    // the filter is opened for them, and a step along the axis makes every propagated sigma the smaller one.
    {
      auto cam = std::make_shared<rebvio::Camera>(a.H, a.W, a.fm, a.fm, a.cx, a.cy);
      auto dcfg = std::make_shared<rebvio::EdgeDetectorConfig>();
      dcfg->keylines_ref = a.kref;
      dcfg->keylines_max = a.kmax;
      rebvio::EdgeDetector detector(cam, dcfg);
      rebvio::io::RawReader src(a.frames, a.H, a.W, 0, 50000);
      rebvio::EdgeMap::SharedPtr maps[2];
      for (int i = 0; i < 2; ++i) {
        rebvio::types::Image img{(uint64_t)i * 50000ull, cv::Mat()};
        src.frame((size_t)i).convertTo(img.data, CV_32FC1, 3.0);
        maps[i] = detector.detect(img);
      }
      const int n0 = maps[0]->size(), n1 = maps[1]->size();
      CHECK(n0 > 100 && n1 > 100);
      rebvio::types::KfHandoverOpts open;
      open.kf_filter.min_matches = 0;
      open.kf_filter.max_rel_sigma = 1e9f;
      rebvio::types::KfPose pose;
      pose.t[2] = 0.1;
      rebvio::KeyframeSnapshot from = maps[0]->keyframeSnapshot(), to = maps[1]->keyframeSnapshot(), twin = maps[1]->keyframeSnapshot();
      CHECK((bool)from && (bool)to && (bool)twin);
      from.addNormals(*maps[0]);
      const std::vector<rebvio::types::CloudPoint> before = from.pointCloud(rebvio::types::CloudFilter{0, 1e9f, 1e-3f, 20.0f});
      std::vector<int> assoc(3, 7), assoc2;
      const rebvio::types::KfHandover h = to.handoverDepth(from, *maps[1], pose, open, &assoc);
      int n_adopted = 0, n_left = 0, n_none = 0;
      for (int v : assoc) {
        CHECK(v == INT_MIN || (v >= -n1 && v < n1));
        n_adopted += v >= 0;
        n_left += v < 0 && v != INT_MIN;
        n_none += v == INT_MIN;
      }
      std::printf("two maps: candidates %d associated %d out_of_range %d claimed %d adopted %d kept %d conflicts %d\n", h.candidates, h.associated,
                  h.out_of_range, h.claimed, h.adopted, h.kept, h.conflicts);
      CHECK((int)assoc.size() == n0 && h.candidates == n0 && h.adopted == n_adopted && h.associated == n0 - n_none &&
            h.associated - h.adopted == n_left);
      CHECK(h.claimed == h.adopted + h.kept + h.conflicts && h.adopted > 12);
      CHECK(to.handoverDepth(from, *maps[1], pose).associated == 0);  // the default filter: nothing has a depth yet
      // src is never written
      const std::vector<rebvio::types::CloudPoint> after = from.pointCloud(rebvio::types::CloudFilter{0, 1e9f, 1e-3f, 20.0f});
      CHECK(before.size() == after.size() && (int)before.size() == n0 &&
            std::memcmp(before.data(), after.data(), before.size() * sizeof(rebvio::types::CloudPoint)) == 0);
      // max_dist -1 is the context's search_range (40)
      rebvio::types::KfHandoverOpts spelled = open;
      spelled.max_dist = 40;
      const rebvio::types::KfHandover g = twin.handoverDepth(from, *maps[1], pose, spelled, &assoc2);
      CHECK(std::memcmp(&g, &h, sizeof(g)) == 0 && assoc2 == assoc);
      rebvio::types::KfHandoverOpts bad = open;
      bad.gate_sigma = 0.0;
      bool refused = false;
      try {
        to.handoverDepth(from, *maps[1], pose, bad);
      } catch (const std::exception&) {
        refused = true;
      }
      CHECK(refused);
      refused = false;
      try {
        to.handoverDepth(to, *maps[1], pose, open);  // dst == src
      } catch (const std::exception&) {
        refused = true;
      }
      CHECK(refused);
      rebvio::KeyframeSnapshot moved = std::move(from);
      CHECK(!from && (bool)moved);
      refused = false;
      try {
        to.handoverDepth(from, *maps[1], pose, open);  // an empty handle
      } catch (const std::exception&) {
        refused = true;
      }
      CHECK(refused);
      moved.reset();
      to.reset();
      twin.reset();
    }
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    ++fails;
  }
  if (fails == 0) std::printf("ok\n");
  return fails ? 1 : 0;
}
