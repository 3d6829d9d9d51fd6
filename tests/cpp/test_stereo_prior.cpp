// rebvio::EdgeMap::fuseStereo and rebvio::Rebvio::setStereo / rightImageCallback / registerStereoPriorCallback on a synthetic stereo
// stream (GPU).
//   test_stereo_prior <left.u8> <right.u8> <W> <H> <N> <fm> <cx> <cy> <keylines_ref> <keylines_max> <imu.bin> <min matches> <baseline>
//                     <z_front> <z_back>
// The class: a detected left map's fresh keylines (rho 1, sigma_rho 20) take the depth of the disparity found in the right frame's
// map (both from one detector here; rebvio::Rebvio below gives the right camera a detector and a backend context of its own) -
// most fused depths lie near one of the scene's two planes, every keyline that is not fused and every other field keeps its
// bits, the right map keeps all of its bits; a missing baseline is refused.
// The pipeline: the stream four times - no stereo call at all; setStereo and a callback but no right image; a right image per
// frame; a right image per frame but one, whose stamp matches no frame. The odometry lines of the first two are byte-identical (a
// frame without a partner runs what it ran). With right images the callback fires once per frame, in frame order, with the frame's
// stamp and fused > 0, and none is dropped. The unmatched image is dropped and counted, and its frame has no callback.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
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
  std::string left, right, imu;
  int W, H, N, kref, kmax, min_matches;
  float fm, cx, cy;
  double baseline, z_front, z_back;
};

struct StereoRec {
  uint64_t ts;
  rebvio::types::StereoPriorCounts counts;
};
struct Run {
  std::vector<std::string> lines;
  std::vector<StereoRec> stereo;
  unsigned dropped = 0;
  bool running = false;
};

// mode 0: nothing of the stereo prior is touched; 1: setStereo and a callback, no right image; 2: a right image per frame; 3: a right
// image per frame, the one of frame `odd` with a stamp of its own
static Run run(const Args& a, int mode, int odd) {
  Run out;
  rebvio::RebvioConfig config;
  config.camera = rebvio::Camera(a.H, a.W, a.fm, a.fm, a.cx, a.cy);
  config.edge_detector.keylines_ref = a.kref;
  config.edge_detector.keylines_max = a.kmax;
  config.core.global_min_matches_threshold = (unsigned)a.min_matches;
  rebvio::io::RawReader src(a.left, a.H, a.W, 0, 50000, a.imu);
  rebvio::io::RawReader right(a.right, a.H, a.W, 0, 50000);
  rebvio::Rebvio rebvio(config);
  std::mutex mu;
  rebvio.registerOdometryCallback([&](rebvio::types::Odometry& o) {
    std::lock_guard<std::mutex> g(mu);
    out.lines.push_back(rebvio::io::OdometryWriter::format(o));
  });
  if (mode >= 1) {
    rebvio::types::StereoPriorOpts so;
    so.baseline = a.baseline;
    rebvio.setStereo(so);
    rebvio.registerStereoPriorCallback([&](uint64_t ts_us, const rebvio::types::StereoPriorCounts& c) {
      std::lock_guard<std::mutex> g(mu);
      out.stereo.push_back(StereoRec{ts_us, c});
    });
  }
  size_t handed = 0;
  rebvio::io::replay(
      src,
      [&](rebvio::types::Image&& im) {
        if (mode >= 2) {
          // at most seven frames ahead of the tracker: none of the eight queued images is pushed out
          while (handed >= (size_t)rebvio.framesProcessed() + 7 && rebvio.running()) std::this_thread::sleep_for(std::chrono::microseconds(100));
          rebvio::types::Image r;
          r.data = right.frame(handed);
          r.ts_us = im.ts_us + ((mode == 3 && (int)handed == odd) ? 7 : 0);
          rebvio.rightImageCallback(std::move(r));
        }
        ++handed;
        rebvio.imageCallback(std::move(im));
      },
      [&](rebvio::types::Imu&& s) { rebvio.imuCallback(std::move(s)); });
  rebvio.waitIdle();
  out.running = rebvio.running();
  out.dropped = rebvio.rightImagesDropped();
  return out;
}

int main(int argc, char** argv) {
  if (argc < 16) return 2;
  Args a;
  a.left = argv[1];
  a.right = argv[2];
  a.W = std::atoi(argv[3]); a.H = std::atoi(argv[4]); a.N = std::atoi(argv[5]);
  a.fm = (float)std::atof(argv[6]); a.cx = (float)std::atof(argv[7]); a.cy = (float)std::atof(argv[8]);
  a.kref = std::atoi(argv[9]); a.kmax = std::atoi(argv[10]);
  a.imu = argv[11];
  a.min_matches = std::atoi(argv[12]);
  a.baseline = std::atof(argv[13]); a.z_front = std::atof(argv[14]); a.z_back = std::atof(argv[15]);
  try {
    // ---- the class --------------------------------------------------------------------------------------------------------------
    {
      auto cam = std::make_shared<rebvio::Camera>(a.H, a.W, a.fm, a.fm, a.cx, a.cy);
      auto dcfg = std::make_shared<rebvio::EdgeDetectorConfig>();
      dcfg->keylines_ref = a.kref;
      dcfg->keylines_max = a.kmax;
      rebvio::EdgeDetector detector(cam, dcfg);
      rebvio::io::RawReader lsrc(a.left, a.H, a.W, 0, 50000), rsrc(a.right, a.H, a.W, 0, 50000);
      rebvio::types::Image li{50000, lsrc.frame(1)}, ri{50000, rsrc.frame(1)};
      rebvio::EdgeMap::SharedPtr map = detector.detect(li), rmap = detector.detect(ri);
      const int n = map->size();
      CHECK(n > 100 && rmap->size() > 100);
      const std::vector<rebvio::types::KeyLine> before = map->keylines(), rbefore = rmap->keylines();
      rebvio::types::StereoPriorOpts so;
      so.baseline = a.baseline;
      std::vector<int> outcome, winner;
      const rebvio::types::StereoPriorCounts c = map->fuseStereo(*rmap, so, &outcome, &winner);
      std::printf("class: n %d usable %d seen %d fused %d gated %d ambiguous %d clamped %d\n", c.candidates, c.usable, c.seen, c.fused, c.gated,
                  c.ambiguous, c.clamped);
      CHECK(c.candidates == n && c.seen == c.fused + c.gated + c.ambiguous && c.usable >= c.seen && c.fused > n / 5 && c.clamped == 0);
      CHECK((int)outcome.size() == n && (int)winner.size() == n);
      const std::vector<rebvio::types::KeyLine>& after = map->keylines();
      int fused = 0, near_plane = 0;
      for (int i = 0; i < n; ++i) {
        rebvio::types::KeyLine x = before[(size_t)i];
        const rebvio::types::KeyLine& y = after[(size_t)i];
        if ((outcome[(size_t)i] & 7) != 1) {
          CHECK(std::memcmp(&x, &y, sizeof(x)) == 0 && winner[(size_t)i] == -1);
          continue;
        }
        ++fused;
        CHECK(winner[(size_t)i] >= 0 && winner[(size_t)i] < rmap->size());
        const double z = 1.0 / y.rho;
        near_plane += std::fabs(z - a.z_front) < 0.1 * a.z_front || std::fabs(z - a.z_back) < 0.1 * a.z_back;
        CHECK(y.sigma_rho > 0.f && y.sigma_rho < 0.2f);
        x.rho = y.rho;
        x.sigma_rho = y.sigma_rho;
        CHECK(std::memcmp(&x, &y, sizeof(x)) == 0);  // nothing else moved, matches included
      }
      CHECK(fused == c.fused);
      std::printf("class: %d of %d fused depths within 10 %% of a plane of the scene\n", near_plane, fused);
      CHECK(near_plane > fused / 2);  // (the median error of a raw stereo depth is about one per cent)
      const std::vector<rebvio::types::KeyLine>& rafter = rmap->keylines();
      CHECK(rafter.size() == rbefore.size() && std::memcmp(rafter.data(), rbefore.data(), rbefore.size() * sizeof(rbefore[0])) == 0);
      // a second pair of maps: the fused one serves as a right map as well
      rebvio::EdgeMap::SharedPtr map2 = detector.detect(li), rmap2 = detector.detect(ri);
      const rebvio::types::StereoPriorCounts c2 = map2->fuseStereo(*rmap2, so);
      CHECK(c2.candidates == map2->size() && c2.fused > 0);
      CHECK(rmap2->fuseStereo(*map, so).candidates == rmap2->size());
      bool refused = false;
      try {
        map2->fuseStereo(*rmap2, rebvio::types::StereoPriorOpts());  // no baseline
      } catch (const std::exception&) {
        refused = true;
      }
      CHECK(refused);
    }
    // ---- the pipeline -------------------------------------------------------------------------------------------------------------
    const Run plain = run(a, 0, -1), idle = run(a, 1, -1), with = run(a, 2, -1), odd = run(a, 3, 5);
    CHECK(plain.running && idle.running && with.running && odd.running);
    CHECK((int)plain.lines.size() == a.N - 1 && plain.lines == idle.lines);
    CHECK(idle.stereo.empty() && idle.dropped == 0 && plain.dropped == 0);
    CHECK((int)with.lines.size() == a.N - 1 && (int)with.stereo.size() == a.N && with.dropped == 0);
    for (size_t k = 0; k < with.stereo.size(); ++k) {
      const StereoRec& r = with.stereo[k];
      CHECK(r.ts == 50000ull * k);
      CHECK(r.counts.candidates > 100 && r.counts.fused > r.counts.candidates / 5 &&
            r.counts.seen == r.counts.fused + r.counts.gated + r.counts.ambiguous);
    }
    std::printf("pipeline: %zu records, %zu fused frames, fused keylines of the first / last %d / %d\n", with.lines.size(), with.stereo.size(),
                with.stereo.empty() ? 0 : with.stereo.front().counts.fused, with.stereo.empty() ? 0 : with.stereo.back().counts.fused);
    // the unmatched stamp: frame 5's right image is 7 us late - no frame has that stamp; it is dropped when frame 6 comes up
    CHECK((int)odd.stereo.size() == a.N - 1 && odd.dropped == 1);
    for (const StereoRec& r : odd.stereo) CHECK(r.ts != 250000ull && r.ts % 50000ull == 0);
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
  if (fails) {
    std::printf("%d checks failed\n", fails);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
