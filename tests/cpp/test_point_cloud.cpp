// rebvio::Rebvio's point-cloud callback and EdgeMap::pointCloud on a synthetic stream (GPU).
//   test_point_cloud <frames.u8> <W> <H> <N> <fm> <cx> <cy> <keylines_ref> <keylines_max> <imu.bin> <min matches> <summary out>
// Runs the stream twice - without and with a registered point-cloud callback - and checks: the odometry lines are byte-identical;
// one cloud per odometry record, right after it, with its stamp; keyline strictly increasing; every value finite; clouds non-empty
// after the warm-up pairs; the cloud of a fresh map through EdgeMap::pointCloud equals the definition applied to its mirror.
// Writes "<ts_us> <count> <first x y z intensity> <last x y z intensity>" (floats as hex bit patterns) per cloud to <summary out>
// for the comparison with rebvio_replay --cloud.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

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
  int W, H, N, kref, kmax, min_matches;
  float fm, cx, cy;
};

struct CloudRec {
  uint64_t ts;
  rebvio::types::CloudPose pose;
  std::vector<rebvio::types::CloudPoint> pts;
  size_t odometry_seen;  // odometry records published when the cloud arrived
};

static rebvio::RebvioConfig make_config(const Args& a) {
  rebvio::RebvioConfig config;
  config.camera = rebvio::Camera(a.H, a.W, a.fm, a.fm, a.cx, a.cy);
  config.edge_detector.keylines_ref = a.kref;
  config.edge_detector.keylines_max = a.kmax;
  config.core.global_min_matches_threshold = (unsigned)a.min_matches;
  return config;
}

static unsigned bits(float v) {
  unsigned w;
  std::memcpy(&w, &v, 4);
  return w;
}

static bool run(const Args& a, bool with_cloud, std::vector<std::string>* lines, std::vector<uint64_t>* odo_ts, std::vector<CloudRec>* clouds) {
  rebvio::RebvioConfig config = make_config(a);
  rebvio::io::RawReader src(a.frames, a.H, a.W, 0, 50000, a.imu);
  rebvio::Rebvio rebvio(config);
  std::mutex mu;
  rebvio.registerOdometryCallback([&](rebvio::types::Odometry& o) {
    std::lock_guard<std::mutex> g(mu);
    lines->push_back(rebvio::io::OdometryWriter::format(o));
    odo_ts->push_back(o.ts_us);
  });
  if (with_cloud)
    rebvio.registerPointCloudCallback([&](const rebvio::types::PointCloud& pc) {
      std::lock_guard<std::mutex> g(mu);
      clouds->push_back(CloudRec{pc.ts_us, pc.pose, std::vector<rebvio::types::CloudPoint>(pc.points, pc.points + pc.size), odo_ts->size()});
    });
  rebvio::io::replay(src, [&](rebvio::types::Image&& im) { rebvio.imageCallback(std::move(im)); },
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
  try {
    std::vector<std::string> plain, with;
    std::vector<uint64_t> ts_plain, ts_with;
    std::vector<CloudRec> none, clouds;
    CHECK(run(a, false, &plain, &ts_plain, &none));
    CHECK(run(a, true, &with, &ts_with, &clouds));
    CHECK((int)plain.size() == a.N - 1 && none.empty());
    CHECK(plain == with);  // byte-identical odometry lines
    CHECK(clouds.size() == with.size());
    size_t nonempty = 0;
    for (size_t i = 0; i < clouds.size() && i < ts_with.size(); ++i) {
      const CloudRec& c = clouds[i];
      CHECK(c.ts == ts_with[i]);
      CHECK(c.odometry_seen == i + 1);  // right after its odometry record, before the next one
      for (size_t k = 0; k < c.pts.size(); ++k) {
        const rebvio::types::CloudPoint& p = c.pts[k];
        if (k) CHECK(p.keyline > c.pts[k - 1].keyline);
        CHECK(p.keyline >= 0 && p.keyline < a.kmax);
        CHECK(std::isfinite(p.xyz[0]) && std::isfinite(p.xyz[1]) && std::isfinite(p.xyz[2]) && std::isfinite(p.rho) &&
              std::isfinite(p.sigma_rho) && std::isfinite(p.gradient_norm));
        CHECK(p.rho >= 1e-3f && p.rho <= 20.0f && p.matches >= 2u && p.sigma_rho <= 0.5f * p.rho);  // the default filter
      }
      if (i >= 6) CHECK(!c.pts.empty());  // after the warm-up pairs
      nonempty += !c.pts.empty();
      for (float v : c.pose.R) CHECK(std::isfinite(v));
      CHECK(std::isfinite(c.pose.scale) && std::isfinite(c.pose.t[0]));
    }
    std::printf("records %zu, clouds %zu (%zu non-empty), last cloud %zu points\n", with.size(), clouds.size(), nonempty,
                clouds.empty() ? (size_t)0 : clouds.back().pts.size());
    if (std::FILE* f = std::fopen(argv[12], "w")) {
      for (const CloudRec& c : clouds) {
        std::fprintf(f, "%llu %zu", (unsigned long long)c.ts, c.pts.size());
        if (!c.pts.empty())
          for (const rebvio::types::CloudPoint* p : {&c.pts.front(), &c.pts.back()})
            std::fprintf(f, " %08x %08x %08x %08x", bits(p->xyz[0]), bits(p->xyz[1]), bits(p->xyz[2]), bits(p->gradient_norm));
        std::fprintf(f, "\n");
      }
      std::fclose(f);
    } else {
      CHECK(!"summary file");
    }

    // EdgeMap::pointCloud (the synchronous form) on a detected map: fresh keylines carry rho = 1, sigma_rho = 20, matches = 0, so a
    // filter that admits them returns every keyline, back-projected as rebvio_hip.h defines it; the default filter returns none
    {
      auto cam = std::make_shared<rebvio::Camera>(a.H, a.W, a.fm, a.fm, a.cx, a.cy);
      auto dcfg = std::make_shared<rebvio::EdgeDetectorConfig>();
      dcfg->keylines_ref = a.kref;
      dcfg->keylines_max = a.kmax;
      rebvio::EdgeDetector detector(cam, dcfg);
      rebvio::io::RawReader src(a.frames, a.H, a.W, 0, 50000);
      rebvio::types::Image img{0, cv::Mat()};
      src.frame(0).convertTo(img.data, CV_32FC1, 3.0);
      rebvio::EdgeMap::SharedPtr map = detector.detect(img);
      CHECK(map->size() > 100);
      CHECK(map->pointCloud().empty());
      rebvio::types::CloudFilter all;
      all.min_matches = 0;
      all.max_rel_sigma = 20.0f;
      rebvio::types::CloudPose pose;
      const float R[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};  // 90 degrees about the optical axis
      for (int i = 0; i < 9; ++i) pose.R[i] = R[i];
      pose.t[2] = 0.25f;
      pose.scale = 2.0f;
      const std::vector<rebvio::types::CloudPoint> pts = map->pointCloud(all, pose);
      CHECK((int)pts.size() == map->size());
      for (size_t i = 0; i < pts.size() && i < (size_t)map->size(); ++i) {
        const rebvio::types::KeyLine& k = (*map)[(int)i];
        const float z = 2.0f / k.rho, xc = k.pos_img[0] / a.fm * z, yc = k.pos_img[1] / a.fm * z;
        CHECK(pts[i].keyline == (int)i && pts[i].rho == k.rho && pts[i].sigma_rho == k.sigma_rho && pts[i].gradient_norm == k.gradient_norm);
        CHECK(pts[i].xyz[0] == -yc && pts[i].xyz[1] == xc && pts[i].xyz[2] == z + 0.25f);
      }
    }
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    ++fails;
  }
  if (fails == 0) std::printf("ok\n");
  return fails ? 1 : 0;
}
