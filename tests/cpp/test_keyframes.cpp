// rebvio::Rebvio's keyframe request and callback, EdgeMap::markKeyframe / keyframeMatches on a synthetic stream (GPU).
//   test_keyframes <frames.u8> <W> <H> <N> <fm> <cx> <cy> <keylines_ref> <keylines_max> <imu.bin> <min matches> <request at frame>
// Runs the stream three times:
//   plain     no keyframe callback, no request
//   callback  a keyframe callback, no request: the odometry lines are byte-identical to plain; one call per odometry record, right
//             after it, with its stamp; kf_matches == 0 everywhere
//   request   the pipeline is drained in front of frame R (waitIdle), requestKeyframe(), the rest is fed: the pair that ends at
//             frame R is the one being tracked when the request is seen, so frame R's map becomes the keyframe - kf_matches == 0
//             up to and including the record of frame R, >= 1 on the next pair and on every pair behind it
// and checks EdgeMap::markKeyframe / keyframeMatches on two detected maps matched through the stepwise calls.
#include <cstdio>
#include <cstdlib>
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

struct KfRec {
  uint64_t ts;
  int kf_matches, keylines;
  size_t odometry_seen;  // odometry records published when the call arrived
};

static bool run(const Args& a, bool with_callback, int request_at, std::vector<std::string>* lines, std::vector<uint64_t>* odo_ts,
                std::vector<KfRec>* recs) {
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
    rebvio.registerKeyframeCallback([&](uint64_t ts_us, int kf_matches, int keylines) {
      std::lock_guard<std::mutex> g(mu);
      recs->push_back(KfRec{ts_us, kf_matches, keylines, odo_ts->size()});
    });
  int fed = 0;
  rebvio::io::replay(src,
                     [&](rebvio::types::Image&& im) {
                       if (fed++ == request_at) {
                         rebvio.waitIdle();  // every pair in front of this frame has been tracked and published
                         rebvio.requestKeyframe();
                       }
                       rebvio.imageCallback(std::move(im));
                     },
                     [&](rebvio::types::Imu&& s) { rebvio.imuCallback(std::move(s)); });
  rebvio.waitIdle();
  return rebvio.running();
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
    std::vector<std::string> plain, with, req;
    std::vector<uint64_t> ts_plain, ts_with, ts_req;
    std::vector<KfRec> none, quiet, marked;
    CHECK(run(a, false, -1, &plain, &ts_plain, &none));
    CHECK(run(a, true, -1, &with, &ts_with, &quiet));
    CHECK((int)plain.size() == a.N - 1 && none.empty());
    CHECK(plain == with);  // byte-identical odometry lines
    CHECK(quiet.size() == with.size());
    for (size_t i = 0; i < quiet.size() && i < ts_with.size(); ++i) {
      CHECK(quiet[i].ts == ts_with[i]);
      CHECK(quiet[i].odometry_seen == i + 1);  // right after its odometry record, before the next one
      CHECK(quiet[i].kf_matches == 0);
      CHECK(quiet[i].keylines > 0 && quiet[i].keylines <= a.kmax);
    }
    CHECK(run(a, true, a.request_at, &req, &ts_req, &marked));
    CHECK(marked.size() == (size_t)a.N - 1 && req.size() == marked.size());
    const uint64_t ts_kf = (uint64_t)a.request_at * 50000ull;
    size_t behind = 0;
    for (const KfRec& r : marked) {
      if (r.ts <= ts_kf) {
        CHECK(r.kf_matches == 0);
      } else {
        CHECK(r.kf_matches >= 1 && r.kf_matches <= r.keylines);
        ++behind;
      }
      std::printf("ts %llu kf_matches %d keylines %d\n", (unsigned long long)r.ts, r.kf_matches, r.keylines);
    }
    CHECK(behind == (size_t)(a.N - 1 - a.request_at));

    // EdgeMap::markKeyframe / keyframeMatches: frame 0 becomes the keyframe and is matched forward into frame 1 by the stepwise
    // calls (minimizeVel leaves the forward matches, forwardMatch hands fields and keyframe ids on)
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
      const int n0 = maps[0]->size(), n1 = maps[1]->size();
      CHECK(n0 > 100 && n1 > 100);
      CHECK(maps[1]->keyframeMatches(n0).empty());  // nothing marked yet
      maps[0]->markKeyframe();
      for (int i = 0; i < n0; ++i) CHECK((*maps[0])[i].match_id_keyframe == i);
      const std::vector<rebvio::types::KfMatch> self = maps[0]->keyframeMatches(n0);
      CHECK((int)self.size() == n0);
      for (size_t i = 0; i < self.size(); ++i) CHECK(self[i].kf_keyline == (int)i && self[i].keyline == (int)i && self[i].claimants == 1);
      core.buildDistanceField(maps[1]);
      rebvio::types::Vector3f vel = TooN::Zeros;
      rebvio::types::Matrix3f Rvel;
      core.minimizeVel(maps[0], vel, Rvel);
      maps[0]->forwardMatch(maps[1]);
      const std::vector<rebvio::types::KfMatch> m = maps[1]->keyframeMatches(n0);
      std::printf("keyframe %d keylines, next frame %d: %zu correspondences\n", n0, n1, m.size());
      CHECK(m.size() > 50 && (int)m.size() <= n0);
      int claimants = 0;
      for (size_t i = 0; i < m.size(); ++i) {
        if (i) CHECK(m[i].kf_keyline > m[i - 1].kf_keyline);  // strictly increasing
        CHECK(m[i].kf_keyline >= 0 && m[i].kf_keyline < n0 && m[i].keyline >= 0 && m[i].keyline < n1 && m[i].claimants >= 1);
        const rebvio::types::KeyLine& k = (*maps[1])[m[i].keyline];
        CHECK(k.match_id_keyframe == m[i].kf_keyline && k.rho == m[i].rho && k.sigma_rho == m[i].sigma_rho && k.matches == m[i].matches &&
              k.pos_img[0] == m[i].pos_img[0] && k.pos_img[1] == m[i].pos_img[1]);
        claimants += m[i].claimants;
      }
      int holders = 0;
      for (int i = 0; i < n1; ++i) holders += (*maps[1])[i].match_id_keyframe >= 0;
      CHECK(claimants == holders);
    }
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    ++fails;
  }
  if (fails == 0) std::printf("ok\n");
  return fails ? 1 : 0;
}
