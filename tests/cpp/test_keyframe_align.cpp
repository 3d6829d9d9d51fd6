// rebvio::Rebvio::setKeyframeAlign and KeyframeSnapshot::addNormals / EdgeMap::keyframeAlign on a synthetic stream (GPU).
//   test_keyframe_align <frames.u8> <W> <H> <N> <fm> <cx> <cy> <keylines_ref> <keylines_max> <imu.bin> <min matches> <request at frame>
// Runs the stream five times, the pipeline drained in front of frame R (waitIdle) and a keyframe requested there:
//   plain    no pose callback
//   chain    a pose callback, setKeyframeAlign off: the poses of the correspondence chain
//   aligned  a pose callback, setKeyframeAlign on: the poses of the alignment through each new map's distance field
//   again    aligned once more
//   late     setKeyframeAlign(true) with no pose callback registered
// The odometry lines of all five are byte-identical. chain and aligned both hand out one pose per odometry record from the keyframe's
// own record on, each right after its record; every aligned pose has candidates = the keyframe's size (the chain's first record
// says it: every keyline of the keyframe is its own correspondence there), finite values, a status of 0, 2 or 3 and, with status 0,
// an orthonormal R and min_used <= used <= candidates; aligned and again are equal in every byte.
// Then KeyframeSnapshot::addNormals / EdgeMap::keyframeAlign on two detected maps: candidates, the association vector against
// `used`, max_dist -1 standing for the context's search_range, an evaluation at a result returning that result's pose, an empty
// snapshot handle refused.
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

struct Run {
  std::vector<std::string> lines;
  std::vector<uint64_t> odo_ts;
  std::vector<PoseRec> recs;
  bool running = false;
};

static Run run(const Args& a, bool with_callback, bool align) {
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
    out.odo_ts.push_back(o.ts_us);
  });
  if (with_callback)
    rebvio.registerKeyframePoseCallback([&](uint64_t ts_us, const rebvio::types::KfPose& p) {
      std::lock_guard<std::mutex> g(mu);
      out.recs.push_back(PoseRec{ts_us, p, out.odo_ts.size()});
    });
  rebvio.setKeyframeAlign(align);
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
  out.running = rebvio.running();
  return out;
}

static bool finite_pose(const rebvio::types::KfPose& p) {
  double v[55];  // R, t, H, g, cost: 55 doubles in a row
  std::memcpy(v, &p, sizeof(v));
  for (int i = 0; i < 55; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
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

static void check_one_pose_per_record(const Args& a, const Run& r) {
  const uint64_t ts_kf = (uint64_t)a.request_at * 50000ull;
  CHECK(r.recs.size() == (size_t)(a.N - a.request_at));  // the keyframe's own record and every record behind it
  for (size_t i = 0; i < r.recs.size(); ++i) {
    const size_t rec = (size_t)a.request_at - 1 + i;  // index of its odometry record
    CHECK(r.recs[i].ts == ts_kf + i * 50000ull);
    CHECK(rec < r.odo_ts.size() && r.odo_ts[rec] == r.recs[i].ts && r.recs[i].odometry_seen == rec + 1);  // right after its record
  }
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
    const Run plain = run(a, false, false), chain = run(a, true, false), aligned = run(a, true, true), again = run(a, true, true),
              late = run(a, false, true);
    CHECK(plain.running && chain.running && aligned.running && again.running && late.running);
    CHECK((int)plain.lines.size() == a.N - 1 && plain.recs.empty() && late.recs.empty());
    CHECK(plain.lines == chain.lines && plain.lines == aligned.lines && plain.lines == again.lines && plain.lines == late.lines);
    check_one_pose_per_record(a, chain);
    check_one_pose_per_record(a, aligned);
    const int kf_size = chain.recs.empty() ? -1 : chain.recs[0].pose.candidates;  // the keyframe against itself: every keyline a candidate
    CHECK(kf_size > 100);
    int ok = 0;
    for (size_t i = 0; i < aligned.recs.size(); ++i) {
      const rebvio::types::KfPose& p = aligned.recs[i].pose;
      const double tn = std::sqrt(p.t[0] * p.t[0] + p.t[1] * p.t[1] + p.t[2] * p.t[2]);
      std::printf("ts %llu status %d candidates %d used %d |t| %.5f cost %.2f", (unsigned long long)aligned.recs[i].ts, p.status, p.candidates, p.used,
                  tn, p.cost);
      if (i < chain.recs.size()) {
        const rebvio::types::KfPose& c = chain.recs[i].pose;
        std::printf("   chain: status %d candidates %d used %d |t| %.5f\n", c.status, c.candidates, c.used,
                    std::sqrt(c.t[0] * c.t[0] + c.t[1] * c.t[1] + c.t[2] * c.t[2]));
      } else {
        std::printf("\n");
      }
      CHECK(p.candidates == kf_size && finite_pose(p));
      CHECK(p.status == 0 || p.status == 2 || p.status == 3);
      CHECK(p.used >= 0 && p.used <= p.candidates);
      if (p.status == 0) {
        CHECK(p.iterations == 8 && p.used >= 12 && from_orthonormal(p) < 1e-12);
        ++ok;
      }
    }
    CHECK(ok > 0);
    CHECK(again.recs.size() == aligned.recs.size());
    for (size_t i = 0; i < aligned.recs.size() && i < again.recs.size(); ++i)
      CHECK(again.recs[i].ts == aligned.recs[i].ts && std::memcmp(&again.recs[i].pose, &aligned.recs[i].pose, sizeof(rebvio::types::KfPose)) == 0);

    // KeyframeSnapshot::addNormals / EdgeMap::keyframeAlign on two detected maps. Fresh maps carry no depth yet (matches 0, the
    // initial sigma_rho): the filter is opened for them.
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
      const int n0 = maps[0]->size();
      CHECK(n0 > 100);
      rebvio::types::KfAlignOpts open;
      open.kf_filter.min_matches = 0;
      open.kf_filter.max_rel_sigma = 1e9f;
      rebvio::KeyframeSnapshot snap = maps[0]->keyframeSnapshot();
      CHECK((bool)snap);
      snap.addNormals(*maps[0]);
      std::vector<int> assoc(3, 7);
      const rebvio::types::KfPose p = maps[1]->keyframeAlign(snap, open, nullptr, &assoc);  // (no chain between the two maps at all)
      int n_assoc = 0;
      for (int v : assoc) {
        CHECK(v >= -1 && v < maps[1]->size());
        n_assoc += v >= 0;
      }
      std::printf("two maps: status %d candidates %d used %d cost %.2f\n", p.status, p.candidates, p.used, p.cost);
      CHECK((int)assoc.size() == n0 && p.candidates == n0 && p.used == n_assoc && p.used > 12 && finite_pose(p));
      CHECK(maps[1]->keyframeAlign(snap).status == 3);  // the default filter: nothing has a depth yet
      // max_dist -1 is the context's search_range, 40 by default
      rebvio::types::KfAlignOpts forty = open;
      forty.max_dist = 40;
      const rebvio::types::KfPose q = maps[1]->keyframeAlign(snap, forty);
      CHECK(std::memcmp(&q, &p, sizeof(q)) == 0);
      // an evaluation at the result: the pose comes back as it went in, with the sums the result carries
      rebvio::types::KfAlignOpts eval = open;
      eval.max_iter = 0;
      const rebvio::types::KfPose at = maps[1]->keyframeAlign(snap, eval, &p);
      CHECK(at.iterations == 0 && std::memcmp(&at, &p, 55 * sizeof(double)) == 0 && at.used == p.used);
      rebvio::types::KfAlignOpts bad = open;
      bad.min_cos = 2.0;
      bool refused = false;
      try {
        maps[1]->keyframeAlign(snap, bad);
      } catch (const std::exception&) {
        refused = true;
      }
      CHECK(refused);
      rebvio::KeyframeSnapshot moved = std::move(snap);
      CHECK(!snap && (bool)moved);
      refused = false;
      try {
        maps[1]->keyframeAlign(snap, open);  // an empty handle
      } catch (const std::exception&) {
        refused = true;
      }
      CHECK(refused);
      refused = false;
      try {
        snap.addNormals(*maps[0]);
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
