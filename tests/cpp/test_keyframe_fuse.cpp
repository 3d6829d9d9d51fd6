// rebvio::Rebvio::setKeyframeDepthFusion / registerKeyframeFuseCallback and KeyframeSnapshot::fuseDepth on a synthetic stream (GPU).
//   test_keyframe_fuse <frames.u8> <W> <H> <N> <fm> <cx> <cy> <keylines_ref> <keylines_max> <imu.bin> <min matches> <request at> <again at>
// Runs the stream six times, the pipeline drained in front of frames R and R2 (waitIdle) and a keyframe requested at each:
//   plain    no callback at all
//   aligned  a pose callback, setKeyframeAlign on, fusion off
//   fused    pose and fuse callbacks, setKeyframeAlign and setKeyframeDepthFusion on
//   again    fused once more
//   noalign  pose and fuse callbacks, fusion on, setKeyframeAlign off
//   nopose   a fuse callback only, both switches on
// The odometry lines of all six are byte-identical. fused hands out one fuse record per pose record of status 0 other than the two
// keyframes' own records, each right after its pose record, with candidates = the keyframe's size and associated = fused + gated +
// flat; up to the first fusion its poses are those of aligned; again equals it in every byte; noalign and nopose hand out none.
// Then KeyframeSnapshot::fuseDepth on two detected maps: the counts against the association vector, the stand-ins pixel_sigma 0 and
// max_dist -1 for the context's values, refusals.
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
  size_t seq;  // position among all pose and fuse calls of the run
};
struct FuseRec {
  uint64_t ts;
  rebvio::types::KfFuse fuse;
  size_t seq;
};

struct Run {
  std::vector<std::string> lines;
  std::vector<PoseRec> poses;
  std::vector<FuseRec> fuses;
  bool running = false;
};

static Run run(const Args& a, bool pose_cb, bool fuse_cb, bool align, bool fusion) {
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
  if (fuse_cb)
    rebvio.registerKeyframeFuseCallback([&](uint64_t ts_us, const rebvio::types::KfFuse& f) {
      std::lock_guard<std::mutex> g(mu);
      out.fuses.push_back(FuseRec{ts_us, f, seq++});
    });
  rebvio.setKeyframeAlign(align);
  rebvio.setKeyframeDepthFusion(fusion);
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
    const Run plain = run(a, false, false, false, false), aligned = run(a, true, false, true, false), fused = run(a, true, true, true, true),
              again = run(a, true, true, true, true), noalign = run(a, true, true, false, true), nopose = run(a, false, true, true, true);
    CHECK(plain.running && aligned.running && fused.running && again.running && noalign.running && nopose.running);
    CHECK((int)plain.lines.size() == a.N - 1);
    CHECK(plain.lines == aligned.lines && plain.lines == fused.lines && plain.lines == again.lines && plain.lines == noalign.lines &&
          plain.lines == nopose.lines);
    CHECK(aligned.fuses.empty() && noalign.fuses.empty() && nopose.fuses.empty() && nopose.poses.empty());
    CHECK(fused.poses.size() == (size_t)(a.N - a.request_at) && aligned.poses.size() == fused.poses.size() &&
          noalign.poses.size() == fused.poses.size());

    // one fuse record per status-0 pose record, except the two keyframes' own; each right behind its pose record
    const uint64_t ts_kf[2] = {(uint64_t)a.request_at * 50000ull, (uint64_t)a.again_at * 50000ull};
    size_t k = 0, first_fused_pose = fused.poses.size();
    int kf_size = -1;
    for (size_t i = 0; i < fused.poses.size(); ++i) {
      const PoseRec& p = fused.poses[i];
      const bool own = p.ts == ts_kf[0] || p.ts == ts_kf[1];
      if (own) kf_size = p.pose.candidates;  // (the alignment's candidates = the snapshot's size)
      std::printf("ts %llu status %d used %d of %d", (unsigned long long)p.ts, p.pose.status, p.pose.used, p.pose.candidates);
      if (own || p.pose.status != 0) {
        std::printf(own ? "   (the keyframe's own record)\n" : "\n");
        CHECK(k >= fused.fuses.size() || fused.fuses[k].ts != p.ts);
        continue;
      }
      CHECK(k < fused.fuses.size());
      if (k >= fused.fuses.size()) break;
      const FuseRec& f = fused.fuses[k++];
      std::printf("   fused: candidates %d associated %d fused %d gated %d flat %d clamped %d\n", f.fuse.candidates, f.fuse.associated, f.fuse.fused,
                  f.fuse.gated, f.fuse.flat, f.fuse.clamped);
      if (first_fused_pose == fused.poses.size()) first_fused_pose = i;
      CHECK(f.ts == p.ts && f.seq == p.seq + 1);
      CHECK(f.fuse.candidates == kf_size && f.fuse.candidates == p.pose.candidates);
      CHECK(f.fuse.associated == f.fuse.fused + f.fuse.gated + f.fuse.flat && f.fuse.associated <= f.fuse.candidates);
      CHECK(f.fuse.fused >= 0 && f.fuse.gated >= 0 && f.fuse.flat >= 0 && f.fuse.clamped >= 0 && f.fuse.clamped <= f.fuse.fused);
    }
    CHECK(k == fused.fuses.size() && k > 0);
    int any = 0;
    for (const FuseRec& f : fused.fuses) any += f.fuse.fused;
    CHECK(any > 0);
    // the record of the second keyframe is a pose record (of its own snapshot) without a fuse record, and fusion goes on behind it
    CHECK(!fused.fuses.empty() && fused.fuses.back().ts > ts_kf[1]);
    for (const FuseRec& f : fused.fuses) CHECK(f.ts != ts_kf[0] && f.ts != ts_kf[1]);
    // up to and including the first fused record the poses are the ones without fusion: the first alignment runs on untouched depths
    for (size_t i = 0; i <= first_fused_pose && i < fused.poses.size() && i < aligned.poses.size(); ++i)
      CHECK(std::memcmp(&fused.poses[i].pose, &aligned.poses[i].pose, sizeof(rebvio::types::KfPose)) == 0);
    // two runs: every byte
    CHECK(again.poses.size() == fused.poses.size() && again.fuses.size() == fused.fuses.size());
    for (size_t i = 0; i < fused.poses.size() && i < again.poses.size(); ++i)
      CHECK(again.poses[i].ts == fused.poses[i].ts && std::memcmp(&again.poses[i].pose, &fused.poses[i].pose, sizeof(rebvio::types::KfPose)) == 0);
    for (size_t i = 0; i < fused.fuses.size() && i < again.fuses.size(); ++i)
      CHECK(again.fuses[i].ts == fused.fuses[i].ts && again.fuses[i].seq == fused.fuses[i].seq &&
            std::memcmp(&again.fuses[i].fuse, &fused.fuses[i].fuse, sizeof(rebvio::types::KfFuse)) == 0);

    // KeyframeSnapshot::fuseDepth on two detected maps. Fresh maps carry no depth yet (matches 0, the initial sigma_rho): the filter
    // is opened for them.
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
      rebvio::types::KfFuseOpts open;
      open.kf_filter.min_matches = 0;
      open.kf_filter.max_rel_sigma = 1e9f;
      rebvio::types::KfPose pose;  // a small sideways step
      pose.t[0] = 0.01;
      rebvio::KeyframeSnapshot snap = maps[0]->keyframeSnapshot(), twin = maps[0]->keyframeSnapshot();
      CHECK((bool)snap && (bool)twin);
      snap.addNormals(*maps[0]);
      twin.addNormals(*maps[0]);
      std::vector<int> assoc(3, 7), assoc2;
      const rebvio::types::KfFuse f = snap.fuseDepth(*maps[1], pose, open, &assoc);
      int n_fused = 0, n_left = 0, n_none = 0;
      for (int v : assoc) {
        CHECK(v == INT_MIN || (v >= -maps[1]->size() && v < maps[1]->size()));
        n_fused += v >= 0;
        n_left += v < 0 && v != INT_MIN;
        n_none += v == INT_MIN;
      }
      std::printf("two maps: candidates %d associated %d fused %d gated %d flat %d clamped %d\n", f.candidates, f.associated, f.fused, f.gated,
                  f.flat, f.clamped);
      CHECK((int)assoc.size() == n0 && f.candidates == n0 && f.fused == n_fused && f.gated + f.flat == n_left && f.associated == n0 - n_none);
      CHECK(f.fused > 12);
      CHECK(snap.fuseDepth(*maps[1], pose).associated == 0);  // the default filter: nothing has a depth yet
      // pixel_sigma 0 and max_dist -1 are the context's pixel_uncertainty (1) and search_range (40)
      rebvio::types::KfFuseOpts spelled = open;
      spelled.pixel_sigma = 1.0;
      spelled.max_dist = 40;
      const rebvio::types::KfFuse g = twin.fuseDepth(*maps[1], pose, spelled, &assoc2);
      CHECK(std::memcmp(&g, &f, sizeof(g)) == 0 && assoc2 == assoc);
      rebvio::types::KfFuseOpts bad = open;
      bad.gate_sigma = 0.0;
      bool refused = false;
      try {
        snap.fuseDepth(*maps[1], pose, bad);
      } catch (const std::exception&) {
        refused = true;
      }
      CHECK(refused);
      rebvio::KeyframeSnapshot moved = std::move(snap);
      CHECK(!snap && (bool)moved);
      refused = false;
      try {
        snap.fuseDepth(*maps[1], pose, open);  // an empty handle
      } catch (const std::exception&) {
        refused = true;
      }
      CHECK(refused);
      moved.reset();
      twin.reset();
    }
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    ++fails;
  }
  if (fails == 0) std::printf("ok\n");
  return fails ? 1 : 0;
}
