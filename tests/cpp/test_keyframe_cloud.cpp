// rebvio::Rebvio::registerKeyframeCloudCallback and KeyframeSnapshot::pointCloud on a synthetic stream (GPU).
//   test_keyframe_cloud <frames.u8> <W> <H> <N> <fm> <cx> <cy> <keylines_ref> <keylines_max> <imu.bin> <min matches> <request at> <again at> <third at>
//   test_keyframe_cloud --read-ply <file>...      prints "<ts_us> <vertices>" per file (io::readPointCloudPly), no GPU
// Runs the stream five times, the pipeline drained in front of the three request frames (waitIdle) and a keyframe requested at each:
//   plain    no callback at all
//   cloud    a keyframe-cloud callback only: the keyframes as marked
//   again    cloud once more
//   fusion   pose and fuse callbacks, setKeyframeAlign and setKeyframeDepthFusion on, no cloud callback
//   fused    fusion with the keyframe-cloud callback: the refined keyframes
// The odometry lines of all five are byte-identical. cloud and fused hand out exactly one cloud per retired keyframe - the first two;
// the third is still current at the end and is not handed out - each right after the odometry record of the pair whose new map takes
// over, with ts_us the retired keyframe's own stamp and the pose R_global, Pos, K of the record it was marked on; keyline strictly
// increasing, every value finite, rho > 0. again equals cloud in every byte; fused differs from cloud where a fusion happened.
// Then KeyframeSnapshot::pointCloud against the queued C entry the callback is served by, on one snapshot with one pose.
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
#include "rebvio_hip.h"

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
  int W, H, N, kref, kmax, min_matches, request_at[3];
  float fm, cx, cy;
};

struct CloudRec {
  uint64_t ts;
  rebvio::types::CloudPose pose;
  std::vector<rebvio::types::CloudPoint> points;
  uint64_t after_record;  // stamp of the odometry record published last when the cloud arrived
};

struct Run {
  std::vector<std::string> lines;
  std::vector<rebvio::types::Odometry> records;
  std::vector<CloudRec> clouds;
  int fused = 0;  // keylines fused over the run
  bool running = false;
};

static Run run(const Args& a, bool cloud_cb, bool fusion) {
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
    out.records.push_back(o);
  });
  if (cloud_cb)
    rebvio.registerKeyframeCloudCallback([&](const rebvio::types::PointCloud& pc) {
      std::lock_guard<std::mutex> g(mu);
      out.clouds.push_back(CloudRec{pc.ts_us, pc.pose, std::vector<rebvio::types::CloudPoint>(pc.points, pc.points + pc.size),
                                    out.records.empty() ? ~0ull : out.records.back().ts_us});
    });
  if (fusion) {
    rebvio.registerKeyframePoseCallback([](uint64_t, const rebvio::types::KfPose&) {});
    rebvio.registerKeyframeFuseCallback([&](uint64_t, const rebvio::types::KfFuse& f) {
      std::lock_guard<std::mutex> g(mu);
      out.fused += f.fused;
    });
    rebvio.setKeyframeAlign(true);
    rebvio.setKeyframeDepthFusion(true);
  }
  int fed = 0;
  rebvio::io::replay(src,
                     [&](rebvio::types::Image&& im) {
                       if (fed == a.request_at[0] || fed == a.request_at[1] || fed == a.request_at[2]) {
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

static bool same_clouds(const Run& x, const Run& y) {
  if (x.clouds.size() != y.clouds.size()) return false;
  for (size_t i = 0; i < x.clouds.size(); ++i) {
    const CloudRec &p = x.clouds[i], &q = y.clouds[i];
    if (p.ts != q.ts || p.after_record != q.after_record || std::memcmp(&p.pose, &q.pose, sizeof(p.pose)) != 0 ||
        p.points.size() != q.points.size() ||
        (!p.points.empty() && std::memcmp(p.points.data(), q.points.data(), p.points.size() * sizeof(rebvio::types::CloudPoint)) != 0))
      return false;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc >= 2 && std::string(argv[1]) == "--read-ply") {
    try {
      for (int i = 2; i < argc; ++i) {
        uint64_t ts = 0;
        const std::vector<rebvio::io::PlyVertex> v = rebvio::io::readPointCloudPly(argv[i], &ts);
        std::printf("%llu %zu\n", (unsigned long long)ts, v.size());
      }
    } catch (const std::exception& e) {
      std::printf("FAIL exception: %s\n", e.what());
      return 1;
    }
    return 0;
  }
  if (argc < 15) return 2;
  Args a;
  a.frames = argv[1];
  a.W = std::atoi(argv[2]); a.H = std::atoi(argv[3]); a.N = std::atoi(argv[4]);
  a.fm = (float)std::atof(argv[5]); a.cx = (float)std::atof(argv[6]); a.cy = (float)std::atof(argv[7]);
  a.kref = std::atoi(argv[8]); a.kmax = std::atoi(argv[9]);
  a.imu = argv[10];
  a.min_matches = std::atoi(argv[11]);
  for (int i = 0; i < 3; ++i) a.request_at[i] = std::atoi(argv[12 + i]);
  try {
    const Run plain = run(a, false, false), cloud = run(a, true, false), again = run(a, true, false), fusion = run(a, false, true),
              fused = run(a, true, true);
    CHECK(plain.running && cloud.running && again.running && fusion.running && fused.running);
    CHECK((int)plain.lines.size() == a.N - 1);
    CHECK(plain.lines == cloud.lines && plain.lines == again.lines && plain.lines == fusion.lines && plain.lines == fused.lines);
    CHECK(plain.clouds.empty() && fusion.clouds.empty());

    uint64_t ts_kf[3];
    for (int i = 0; i < 3; ++i) ts_kf[i] = (uint64_t)a.request_at[i] * 50000ull;
    for (const Run* r : {&cloud, &fused}) {
      // one cloud per retired keyframe: the first two; the third is still current when processing ends
      CHECK(r->clouds.size() == 2);
      for (size_t k = 0; k < r->clouds.size() && k < 2; ++k) {
        const CloudRec& c = r->clouds[k];
        std::printf("%s: keyframe %llu retired behind record %llu: %zu points\n", r == &cloud ? "cloud" : "fused", (unsigned long long)c.ts,
                    (unsigned long long)c.after_record, c.points.size());
        CHECK(c.ts == ts_kf[k]);                  // the keyframe's own stamp ...
        CHECK(c.after_record == ts_kf[k + 1]);    // ... delivered with the record of the map that takes over
        // the pose: R_global, Pos, K of the record the keyframe was marked on
        const rebvio::types::Odometry* rec = nullptr;
        for (const rebvio::types::Odometry& o : r->records)
          if (o.ts_us == c.ts) rec = &o;
        CHECK(rec != nullptr);
        if (rec) {
          CHECK(c.pose.t[0] == (float)rec->position[0] && c.pose.t[1] == (float)rec->position[1] && c.pose.t[2] == (float)rec->position[2]);
          CHECK(c.pose.scale == (float)rec->scale);
          const rebvio::types::Matrix3f Rg = TooN::SO3<rebvio::types::Float>(rec->orientation).get_matrix();
          for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) CHECK(std::fabs(c.pose.R[3 * i + j] - Rg(i, j)) < 1e-5f);  // (through ln and exp)
        }
        CHECK(!c.points.empty());
        int last = -1;
        for (const rebvio::types::CloudPoint& p : c.points) {
          CHECK(p.keyline > last && p.keyline < a.kmax);
          last = p.keyline;
          CHECK(std::isfinite(p.xyz[0]) && std::isfinite(p.xyz[1]) && std::isfinite(p.xyz[2]) && std::isfinite(p.sigma_rho));
          CHECK(p.rho > 0.0f && std::isfinite(p.rho) && p.matches >= 2u);
          CHECK(p.gradient_norm == 0.0f && !std::signbit(p.gradient_norm));
        }
      }
    }
    CHECK(same_clouds(cloud, again));  // two runs: every byte
    // the refined keyframe: where keylines were fused the cloud is not the keyframe as marked (same stamps and poses)
    std::printf("keylines fused over the run: %d\n", fused.fused);
    CHECK(fused.fused == fusion.fused);
    if (fused.fused > 0) CHECK(!same_clouds(cloud, fused));
    for (size_t k = 0; k < cloud.clouds.size() && k < fused.clouds.size(); ++k)
      CHECK(cloud.clouds[k].ts == fused.clouds[k].ts && std::memcmp(&cloud.clouds[k].pose, &fused.clouds[k].pose, sizeof(rebvio::types::CloudPose)) == 0);

    // KeyframeSnapshot::pointCloud = what the callback is served by (the queued entry), for the same snapshot, filter and pose.
    // Fresh maps carry no depth yet (matches 0, the initial sigma_rho): the filter is opened for them.
    {
      auto cam = std::make_shared<rebvio::Camera>(a.H, a.W, a.fm, a.fm, a.cx, a.cy);
      auto dcfg = std::make_shared<rebvio::EdgeDetectorConfig>();
      dcfg->keylines_ref = a.kref;
      dcfg->keylines_max = a.kmax;
      rebvio::EdgeDetector detector(cam, dcfg);
      rebvio::io::RawReader src(a.frames, a.H, a.W, 0, 50000);
      rebvio::types::Image img{0ull, cv::Mat()};
      src.frame(0).convertTo(img.data, CV_32FC1, 3.0);
      rebvio::EdgeMap::SharedPtr map = detector.detect(img);
      const int n0 = map->size();
      CHECK(n0 > 100);
      rebvio::KeyframeSnapshot snap = map->keyframeSnapshot();
      rebvio::types::CloudFilter open;
      open.min_matches = 0;
      open.max_rel_sigma = 1e9f;
      const rebvio::types::CloudPose pose = cloud.clouds.empty() ? rebvio::types::CloudPose() : cloud.clouds[0].pose;
      CHECK(snap.pointCloud().empty());  // the default filter: nothing has a depth yet
      const std::vector<rebvio::types::CloudPoint> got = snap.pointCloud(open, pose);
      CHECK((int)got.size() == n0);
      rebvio_hip_cloud* cl = nullptr;
      CHECK(rebvio_hip_kf_snapshot_point_cloud_async(snap.handle(), reinterpret_cast<const rebvio_hip_cloud_filter*>(&open),
                                                     reinterpret_cast<const rebvio_hip_cloud_pose*>(&pose), &cl) == 0);
      const rebvio_hip_cloud_point* pts = nullptr;
      int n = 0;
      CHECK(cl && rebvio_hip_cloud_wait(cl, &pts, &n, nullptr) == 0);
      CHECK(n == (int)got.size() && pts && std::memcmp(pts, got.data(), got.size() * sizeof(rebvio::types::CloudPoint)) == 0);
      rebvio_hip_cloud_release(cl);
      // the map's own cloud shows the same keylines at the same places (it carries the gradient norm, the snapshot's does not)
      const std::vector<rebvio::types::CloudPoint> of_map = map->pointCloud(open, pose);
      CHECK(of_map.size() == got.size());
      for (size_t i = 0; i < got.size() && i < of_map.size(); ++i)
        CHECK(std::memcmp(of_map[i].xyz, got[i].xyz, 12) == 0 && of_map[i].keyline == got[i].keyline && of_map[i].rho == got[i].rho);
      rebvio::KeyframeSnapshot moved = std::move(snap);
      bool refused = false;
      try {
        snap.pointCloud();  // an empty handle
      } catch (const std::exception&) {
        refused = true;
      }
      CHECK(refused && (int)moved.pointCloud(open).size() == n0);
    }
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    ++fails;
  }
  if (fails == 0) std::printf("ok\n");
  return fails ? 1 : 0;
}
