// rebvio::EdgeMap::fuseDepthImage and rebvio::Rebvio::depthImageCallback / setDepthPrior / registerDepthPriorCallback on a synthetic
// stream with rendered depth images (GPU).
//   test_depth_prior <frames.u8> <depth.u16> <W> <H> <N> <fm> <cx> <cy> <keylines_ref> <keylines_max> <imu.bin> <min matches>
// The class: a detected map's fresh keylines (rho 1, sigma_rho 20) take the sensor's depth - every fused keyline's new depth lies
// among the depths of the image around it, every other keyline and every other field keeps its bits; DepthImage::unit replaces the
// options' unit; a second map handed the image as float metres gets the same counts; a wrong size is refused.
// The pipeline: the stream four times - no depth call at all; a depth-prior callback registered but no image handed in; an image per
// frame; an image per frame but one, whose stamp matches no frame. The odometry lines of the first two are byte-identical (a frame
// without an image runs what it ran). With images the callback fires once per frame, in frame order, with the frame's stamp and
// fused > 0, and none is dropped (the pose is not integrated before the fifteenth frame: the odometry lines of so short a stream say
// nothing about the depths). The unmatched image is dropped and counted, and its frame has no callback.
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
  std::string frames, depth, imu;
  int W, H, N, kref, kmax, min_matches;
  float fm, cx, cy;
};

struct DepthRec {
  uint64_t ts;
  rebvio::types::DepthPriorCounts counts;
};
struct Run {
  std::vector<std::string> lines;
  std::vector<rebvio::types::Odometry> odometry;
  std::vector<DepthRec> depth;
  unsigned dropped = 0;
  bool running = false;
};

static std::vector<uint16_t> read_depth(const Args& a) {
  std::vector<uint16_t> d((size_t)a.N * a.W * a.H);
  std::FILE* f = std::fopen(a.depth.c_str(), "rb");
  if (!f || std::fread(d.data(), 2, d.size(), f) != d.size()) {
    std::printf("cannot read %s\n", a.depth.c_str());
    std::exit(2);
  }
  std::fclose(f);
  return d;
}

// mode 0: nothing of the depth prior is touched; 1: callback and options, no image; 2: an image per frame; 3: an image per frame, the
// one of frame `odd` with a stamp of its own
static Run run(const Args& a, const std::vector<uint16_t>& depth, int mode, int odd) {
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
    out.odometry.push_back(o);
  });
  if (mode >= 1) {
    rebvio.setDepthPrior(rebvio::types::DepthPriorOpts());
    rebvio.registerDepthPriorCallback([&](uint64_t ts_us, const rebvio::types::DepthPriorCounts& c) {
      std::lock_guard<std::mutex> g(mu);
      out.depth.push_back(DepthRec{ts_us, c});
    });
  }
  size_t handed = 0;
  rebvio::io::replay(
      src,
      [&](rebvio::types::Image&& im) {
        if (mode >= 2) {
          // at most seven frames ahead of the tracker: none of the eight queued images is pushed out
          while (handed >= (size_t)rebvio.framesProcessed() + 7 && rebvio.running()) std::this_thread::sleep_for(std::chrono::microseconds(100));
          rebvio::types::DepthImage d;
          d.data = depth.data() + handed * (size_t)a.W * a.H;
          d.rows = a.H;
          d.cols = a.W;
          d.format = rebvio::types::DEPTH_U16;
          d.ts_us = im.ts_us + ((mode == 3 && (int)handed == odd) ? 7 : 0);
          rebvio.depthImageCallback(std::move(d));
        }
        ++handed;
        rebvio.imageCallback(std::move(im));
      },
      [&](rebvio::types::Imu&& s) { rebvio.imuCallback(std::move(s)); });
  rebvio.waitIdle();
  out.running = rebvio.running();
  out.dropped = rebvio.depthImagesDropped();
  return out;
}

int main(int argc, char** argv) {
  if (argc < 13) return 2;
  Args a;
  a.frames = argv[1];
  a.depth = argv[2];
  a.W = std::atoi(argv[3]); a.H = std::atoi(argv[4]); a.N = std::atoi(argv[5]);
  a.fm = (float)std::atof(argv[6]); a.cx = (float)std::atof(argv[7]); a.cy = (float)std::atof(argv[8]);
  a.kref = std::atoi(argv[9]); a.kmax = std::atoi(argv[10]);
  a.imu = argv[11];
  a.min_matches = std::atoi(argv[12]);
  try {
    const std::vector<uint16_t> depth = read_depth(a);
    // ---- the class --------------------------------------------------------------------------------------------------------------
    {
      auto cam = std::make_shared<rebvio::Camera>(a.H, a.W, a.fm, a.fm, a.cx, a.cy);
      auto dcfg = std::make_shared<rebvio::EdgeDetectorConfig>();
      dcfg->keylines_ref = a.kref;
      dcfg->keylines_max = a.kmax;
      rebvio::EdgeDetector detector(cam, dcfg);
      rebvio::io::RawReader src(a.frames, a.H, a.W, 0, 50000);
      rebvio::types::Image img{0, cv::Mat()};
      src.frame(1).convertTo(img.data, CV_32FC1, 3.0);
      rebvio::EdgeMap::SharedPtr map = detector.detect(img);
      const int n = map->size();
      CHECK(n > 100);
      const std::vector<rebvio::types::KeyLine> before = map->keylines();
      const uint16_t* d1 = depth.data() + (size_t)a.W * a.H;
      rebvio::types::DepthImage di;
      di.data = d1;
      di.rows = a.H;
      di.cols = a.W;
      di.format = rebvio::types::DEPTH_U16;
      di.ts_us = 50000;
      std::vector<int> outcome;
      const rebvio::types::DepthPriorCounts c = map->fuseDepthImage(di, rebvio::types::DepthPriorOpts(), &outcome);
      std::printf("class: n %d sampled %d fused %d gated %d jumps %d clamped %d\n", c.candidates, c.sampled, c.fused, c.gated, c.jumps, c.clamped);
      CHECK(c.candidates == n && c.sampled == c.fused + c.gated && c.fused > n / 2 && c.gated == 0 && c.clamped == 0 && c.jumps > 0);
      CHECK((int)outcome.size() == n);
      const std::vector<rebvio::types::KeyLine>& after = map->keylines();
      int fused = 0;
      for (int i = 0; i < n; ++i) {
        rebvio::types::KeyLine x = before[(size_t)i];
        const rebvio::types::KeyLine& y = after[(size_t)i];
        if ((outcome[(size_t)i] & 3) != 1) {
          CHECK(std::memcmp(&x, &y, sizeof(x)) == 0);
          continue;
        }
        ++fused;
        // the depths of the image within three pixels of the keyline bracket the new depth (a fresh keyline takes the sensor's)
        const int px = (int)std::floor(x.pos[0] + 0.5f), py = (int)std::floor(x.pos[1] + 0.5f);
        double lo = 1e30, hi = 0.0;
        for (int yy = std::max(0, py - 3); yy <= std::min(a.H - 1, py + 3); ++yy)
          for (int xx = std::max(0, px - 3); xx <= std::min(a.W - 1, px + 3); ++xx) {
            const double z = d1[(size_t)yy * a.W + xx] * 0.001;
            if (z > 0.0) {
              lo = std::min(lo, z);
              hi = std::max(hi, z);
            }
          }
        CHECK(1.0 / y.rho >= lo * 0.999 && 1.0 / y.rho <= hi * 1.001);
        CHECK(y.sigma_rho > 0.f && y.sigma_rho < 0.01f);
        x.rho = y.rho;
        x.sigma_rho = y.sigma_rho;
        CHECK(std::memcmp(&x, &y, sizeof(x)) == 0);  // nothing else moved, matches included
      }
      CHECK(fused == c.fused);
      // DepthImage::unit replaces the options' unit: counts of 2 mm, every depth doubled
      rebvio::EdgeMap::SharedPtr map2 = detector.detect(img);
      di.unit = 0.002;
      const rebvio::types::DepthPriorCounts c2 = map2->fuseDepthImage(di);
      CHECK(c2.sampled == c.sampled && c2.fused == c.fused);
      const std::vector<rebvio::types::KeyLine>& doubled = map2->keylines();
      for (int i = 0; i < n; ++i)
        if ((outcome[(size_t)i] & 3) == 1) CHECK(std::fabs(doubled[(size_t)i].rho * 2.0f - after[(size_t)i].rho) < 1e-4f * after[(size_t)i].rho);
      // the same image as float metres, with a pitch
      rebvio::EdgeMap::SharedPtr map3 = detector.detect(img);
      std::vector<float> metres((size_t)a.H * (a.W + 3), 1.0f);
      for (int yy = 0; yy < a.H; ++yy)
        for (int xx = 0; xx < a.W; ++xx) metres[(size_t)yy * (a.W + 3) + xx] = (float)(d1[(size_t)yy * a.W + xx] * 0.001);
      rebvio::types::DepthImage df;
      df.data = metres.data();
      df.rows = a.H;
      df.cols = a.W;
      df.pitch = (size_t)(a.W + 3) * sizeof(float);
      df.format = rebvio::types::DEPTH_F32;
      const rebvio::types::DepthPriorCounts c3 = map3->fuseDepthImage(df);
      CHECK(c3.sampled == c.sampled && c3.fused == c.fused && c3.jumps == c.jumps);
      bool refused = false;
      try {
        df.cols = a.W - 1;
        map3->fuseDepthImage(df);
      } catch (const std::exception&) {
        refused = true;
      }
      CHECK(refused);
    }
    // ---- the pipeline -------------------------------------------------------------------------------------------------------------
    const Run plain = run(a, depth, 0, -1), idle = run(a, depth, 1, -1), with = run(a, depth, 2, -1), odd = run(a, depth, 3, 5);
    CHECK(plain.running && idle.running && with.running && odd.running);
    CHECK((int)plain.lines.size() == a.N - 1 && plain.lines == idle.lines);
    CHECK(idle.depth.empty() && idle.dropped == 0 && plain.dropped == 0);
    CHECK((int)with.lines.size() == a.N - 1 && (int)with.depth.size() == a.N && with.dropped == 0);
    for (size_t k = 0; k < with.depth.size(); ++k) {
      const DepthRec& r = with.depth[k];
      CHECK(r.ts == 50000ull * k);
      CHECK(r.counts.candidates > 100 && r.counts.fused > r.counts.candidates / 2 && r.counts.sampled == r.counts.fused + r.counts.gated);
    }
    CHECK(with.lines.size() == plain.lines.size());  // (what the prior does to the tracker: tests/test_depth_prior_gpu.py, bit for bit)
    std::printf("pipeline: %zu records, %zu fused frames, fused keylines of the first / last %d / %d\n", with.lines.size(), with.depth.size(),
                with.depth.empty() ? 0 : with.depth.front().counts.fused, with.depth.empty() ? 0 : with.depth.back().counts.fused);
    // the unmatched stamp: frame 5's image is 7 us late - no frame has that stamp; it is dropped when frame 6 comes up
    CHECK((int)odd.depth.size() == a.N - 1 && odd.dropped == 1);
    for (const DepthRec& r : odd.depth) CHECK(r.ts != 250000ull && r.ts % 50000ull == 0);
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
