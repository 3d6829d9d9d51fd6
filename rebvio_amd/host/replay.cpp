// rebvio_replay: run rebvio::Rebvio over a dataset on disk and write the odometry in the reference's regression format.
//   rebvio_replay --asl <mav0 dir> --euroc --out odometry.txt [--first N --count M] [--colour]
//   rebvio_replay --raw frames.u8 --size W H [--imu imu.bin] [--dt 50000] [--camera fm cx cy [k1 k2 p1 p2 k3]] --out odometry.txt
// --euroc selects the reference's built-in EuRoC MH cam0 model (camera.hpp:25-45). With the real MH_03 data
// (first = the frame at 15 s) this replays what ros_rebvio/test/test_ros_rebvio.cpp checks against its golden file.
// --colour: RGB(A) PNG frames go to rebvio::Rebvio as CV_8UC3 / CV_8UC4 (OpenCV's channel order) and are converted to grey on the
// device, instead of to luma while they are read; the odometry is the same.
// --mask mask.png: a grey PNG of the frames' size as the detection mask (Rebvio::setDetectionMask): keylines come only from pixels
// whose byte is non-zero (in undistorted coordinates when a lens model is given).
// --cloud PREFIX: every published record's point cloud (Rebvio::registerPointCloudCallback, default filter) as a binary
// little-endian PLY file PREFIX<ts_us>.ply with the vertex properties x, y, z, intensity (io::writePointCloudPly).
// --cloud-dry: the callback is registered and counts points, no file is written (what the callback costs the pipeline:
// tools/cloud_rate.py).
// --polylines PREFIX [--min-chain N]: every published record's edge polylines (Rebvio::registerEdgePolylineCallback, default filter,
// chains of at least N members, default 8) as PREFIX<ts_us>.ply: the cloud's vertex element plus `element edge` (io::writePolylinesPly).
// --segments PREFIX [--seg-tol T]: every published record's straight segments (Rebvio::registerEdgeSegmentCallback, the default
// options with --min-chain's N and a split tolerance of T px, 0..1000, default 1) as PREFIX<ts_us>.ply: two vertices and one edge per
// depth-valid segment (io::writeSegmentsPly). The odometry file is what it is without it.
// --kf-pose FILE [--kf-every N]: the pose of every tracked map relative to the keyframe (Rebvio::registerKeyframePoseCallback), one
// line per record that has one: ts_us status used R (9 values, row-major) t (3 values). A keyframe is requested before the first
// frame and again after every N-th record (default 10).
// --kf-align FILE [--kf-every N]: the same file, from the alignment of the keyframe to every tracked map through the map's distance
// field (Rebvio::setKeyframeAlign) instead of the correspondence chain. One of --kf-pose and --kf-align.
// --kf-window N FILE: needs --kf-align. Keeps the last N (1..15) retired keyframes aligned to every tracked map next to the current one
// (Rebvio::setKeyframeWindow, Rebvio::registerKeyframeWindowCallback) and writes one line per (record, keyframe) - the current keyframe
// first, then the window's members, newest first: ts_us kf_ts_us status used inliers R (9 values, row-major) t (3 values), doubles
// as %.17g. The odometry file and the --kf-align file are what they are without it.
// --kf-fuse FILE [--kf-every N]: implies the alignment (with or without --kf-align FILE; not with --kf-pose) and fuses every aligned
// map into the keyframe snapshot (Rebvio::setKeyframeDepthFusion), one line per fusion, i.e. per pose record of status 0 other than
// the keyframe's own: ts_us candidates associated fused gated flat clamped.
// --kf-handover FILE: needs --kf-align. Hands every retired keyframe's refined depths on to its successor
// (Rebvio::setKeyframeDepthHandover, Rebvio::registerKeyframeHandoverCallback), one line per hand-over: ts_us kf_ts_us candidates
// associated out_of_range claimed adopted kept conflicts - ts_us the record's stamp, kf_ts_us the retired keyframe's own.
// --kf-cloud PREFIX [--kf-every N]: every retired keyframe's point cloud (Rebvio::registerKeyframeCloudCallback, default filter) as
// PREFIX<ts_us>.ply, ts_us the keyframe's own stamp, through the same PLY writer; keyframes are requested as for --kf-pose. Alone it
// writes the keyframes as marked; with --kf-fuse (and --kf-align) the refined ones. The keyframe current at the end is not written.
// --places FILE [--place-exclude N] [--kf-every N]: place recognition (Rebvio::setPlaceRecognition with room for 4096 keyframes, the
// default top_k and max_distance, exclude_last = N, default 10; Rebvio::registerPlaceCallback), one line per match: ts_us tag distance
// index - ts_us the record whose map was marked, tag the stamp of the keyframe it looks like, index that keyframe's row in the
// database. Keyframes are requested as for --kf-pose. The summary on stderr counts the queries and the matches. The odometry file is
// what it is without it.
// --depth FILE [--depth-unit U]: registered depth images, one per frame in frame order (frame 0 of the file belongs to frame 0 of the
// stream, whatever --first is), raw little-endian uint16 counts of U metres (default 0.001; 0 = no depth), W x H each, dense. Every
// frame's image is handed to Rebvio::depthImageCallback in front of the frame itself; the reader then stays at most seven frames
// ahead of the tracker, so that none of the eight queued images is pushed out. The summary on stderr counts the images, the fused frames and keylines.
// --right FILE|DIR --baseline B: the right camera of a rectified stereo pair through the same readers as the left stream - with --raw a
// raw file of W x H frames, with --asl a mav0 folder whose cam1 is read - frame i belonging to left frame i and taking its stamp; B
// metres from the left camera to the right one along the left camera's x axis. The right frames are assumed rectified to the left
// ones. Every right frame is handed to Rebvio::rightImageCallback in front of its left frame (Rebvio::setStereo with the default
// options and B), the reader staying at most seven frames ahead of the tracker. The summary on stderr counts the images, the fused
// frames and keylines.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "rebvio/io/stream_io.hpp"
#include "rebvio/rebvio.hpp"

int main(int argc, char** argv) {
  std::string asl, raw, imu, out, mask_png, cloud_prefix, kf_pose_path, kf_fuse_path, kf_cloud_prefix, kf_window_path, kf_handover_path;
  std::string polylines_prefix, depth_path, right_path, places_path;
  int place_exclude = 10;
  double depth_unit = 0.001, baseline = 0.0;
  int min_chain = 8;
  std::string segments_prefix;
  double seg_tol = 1.0;
  bool have_seg_tol = false;
  int kf_window = 0;
  bool kf_align = false;
  int kf_every = 10;
  int W = 0, H = 0;
  size_t first = 0, count = (size_t)-1;
  uint64_t dt = 50000;
  bool euroc = false, colour = false, cloud_dry = false;
  float cam[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int ncam = 0, kref = 0, kmax = 0, min_matches = -1;
  auto usage = [&]() {
    std::fprintf(stderr, "usage: %s (--asl mav0 [--colour] | --raw frames.u8 --size W H [--imu imu.bin]) [--euroc | --camera fm cx cy [k1 k2 p1 p2 k3]] "
                 "[--mask mask.png] [--depth FILE [--depth-unit U]] [--right FILE|DIR --baseline B] [--cloud PREFIX | --cloud-dry] [--polylines PREFIX [--min-chain N]] [--segments PREFIX [--seg-tol T]] [(--kf-pose | --kf-align) FILE [--kf-every N]] [--kf-fuse FILE] [--kf-handover FILE] [--kf-cloud PREFIX] [--places FILE [--place-exclude N]] --out file\n", argv[0]);
    return 2;
  };
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    auto next = [&]() -> const char* {
      if (i + 1 >= argc) {
        std::fprintf(stderr, "missing value after %s\n", a.c_str());
        std::exit(2);
      }
      return argv[++i];
    };
    if (a == "--asl") asl = next();
    else if (a == "--raw") raw = next();
    else if (a == "--imu") imu = next();
    else if (a == "--out") out = next();
    else if (a == "--size") { W = std::atoi(next()); H = std::atoi(next()); }
    else if (a == "--first") first = (size_t)std::atoll(next());
    else if (a == "--count") count = (size_t)std::atoll(next());
    else if (a == "--dt") dt = (uint64_t)std::atoll(next());
    else if (a == "--euroc") euroc = true;
    else if (a == "--colour") colour = true;
    else if (a == "--mask") {
      if (i + 1 >= argc || std::strncmp(argv[i + 1], "--", 2) == 0) return usage();
      mask_png = argv[++i];
    }
    else if (a == "--depth") depth_path = next();
    else if (a == "--depth-unit") depth_unit = std::atof(next());
    else if (a == "--right") right_path = next();
    else if (a == "--baseline") baseline = std::atof(next());
    else if (a == "--cloud") cloud_prefix = next();
    else if (a == "--cloud-dry") cloud_dry = true;
    else if (a == "--polylines") {
      if (!polylines_prefix.empty()) return usage();
      polylines_prefix = next();
    }
    else if (a == "--min-chain") min_chain = std::atoi(next());
    else if (a == "--segments") {
      if (!segments_prefix.empty()) return usage();
      segments_prefix = next();
    }
    else if (a == "--seg-tol") {
      if (have_seg_tol) return usage();
      have_seg_tol = true;
      const char* text = next();
      char* end = nullptr;
      seg_tol = std::strtod(text, &end);
      if (end == text || *end != 0) return usage();  // not a number
    }
    else if (a == "--kf-pose" || a == "--kf-align") {
      if (!kf_pose_path.empty()) return usage();  // one of the two, once
      kf_align = a == "--kf-align";
      kf_pose_path = next();
    }
    else if (a == "--kf-fuse") {
      if (!kf_fuse_path.empty()) return usage();
      kf_fuse_path = next();
    }
    else if (a == "--kf-handover") {
      if (!kf_handover_path.empty()) return usage();
      kf_handover_path = next();
    }
    else if (a == "--kf-window") {
      if (!kf_window_path.empty()) return usage();
      kf_window = std::atoi(next());
      kf_window_path = next();
    }
    else if (a == "--kf-cloud") kf_cloud_prefix = next();
    else if (a == "--kf-every") kf_every = std::atoi(next());
    else if (a == "--places") {
      if (!places_path.empty()) return usage();
      places_path = next();
    }
    else if (a == "--place-exclude") place_exclude = std::atoi(next());
    else if (a == "--keylines") { kref = std::atoi(next()); kmax = std::atoi(next()); }
    else if (a == "--min-matches") min_matches = std::atoi(next());
    else if (a == "--camera") {
      while (ncam < 8 && i + 1 < argc && (std::isdigit((unsigned char)argv[i + 1][0]) || argv[i + 1][0] == '-' || argv[i + 1][0] == '.') &&
             std::strncmp(argv[i + 1], "--", 2) != 0)
        cam[ncam++] = (float)std::atof(argv[++i]);
    } else {
      std::fprintf(stderr, "unknown option %s\n", a.c_str());
      return 2;
    }
  }
  if ((asl.empty() == raw.empty()) || out.empty() || kf_every < 1 || min_chain < 1 || !(depth_unit > 0.0)) return usage();
  if (right_path.empty() != !(baseline > 0.0)) return usage();  // --right and --baseline come together
  if (!(seg_tol >= 0.0 && seg_tol <= 1000.0) || (have_seg_tol && segments_prefix.empty())) return usage();  // --seg-tol: 0..1000 px, with --segments
  if (place_exclude < 0) return usage();
  if (!kf_window_path.empty() && (!kf_align || kf_pose_path.empty() || kf_window < 1 || kf_window > 15)) return usage();  // needs --kf-align FILE
  if (!kf_handover_path.empty() && (!kf_align || kf_pose_path.empty())) return usage();  // needs --kf-align FILE
  if (!kf_fuse_path.empty()) {  // the fusion runs behind the alignment only
    if (!kf_pose_path.empty() && !kf_align) return usage();
    kf_align = true;
  }
  try {
    std::unique_ptr<rebvio::io::StreamSource> src;
    if (!asl.empty()) src.reset(new rebvio::io::EurocReader(asl, "cam0", "imu0", colour));
    else src.reset(new rebvio::io::RawReader(raw, H, W, 0, dt, imu));
    if (src->numFrames() == 0) {
      std::fprintf(stderr, "no frames\n");
      return 1;
    }
    if (W == 0) {
      const cv::Mat f0 = src->frame(0);
      W = f0.cols;
      H = f0.rows;
    }
    rebvio::RebvioConfig config;
    if (!euroc) {
      const float fm = ncam > 0 ? cam[0] : 458.0f * W / 640.0f;
      config.camera = rebvio::Camera(H, W, fm, fm, ncam > 1 ? cam[1] : W / 2.0f, ncam > 2 ? cam[2] : H / 2.0f);
      if (ncam > 3) config.camera.k1_ = cam[3];
      if (ncam > 4) config.camera.k2_ = cam[4];
      if (ncam > 5) config.camera.p1_ = cam[5];
      if (ncam > 6) config.camera.p2_ = cam[6];
      if (ncam > 7) config.camera.k3_ = cam[7];
    }
    if (kref > 0) {
      config.edge_detector.keylines_ref = kref;
      config.edge_detector.keylines_max = kmax;
    }
    if (min_matches >= 0) config.core.global_min_matches_threshold = (unsigned)min_matches;
    rebvio::io::OdometryWriter writer(out);
    rebvio::Rebvio rebvio(config);
    if (!mask_png.empty()) {
      const rebvio::io::PngPixels m = rebvio::io::readPngPixels(mask_png);
      if (m.format != REBVIO_HIP_PX_GRAY8) {
        std::fprintf(stderr, "error: mask %s is not a grey PNG\n", mask_png.c_str());
        return 1;
      }
      if (m.data.rows != H || m.data.cols != W) {
        std::fprintf(stderr, "error: mask %s is %dx%d, the frames are %dx%d\n", mask_png.c_str(), m.data.cols, m.data.rows, W, H);
        return 1;
      }
      rebvio.setDetectionMask(m.data);
    }
    std::mutex mu;
    const bool want_kf = !kf_pose_path.empty() || !kf_fuse_path.empty();
    size_t n_odo = 0;
    std::chrono::steady_clock::time_point t_first, t_last;
    rebvio.registerOdometryCallback([&](rebvio::types::Odometry& o) {
      std::lock_guard<std::mutex> g(mu);
      writer.write(o);
      t_last = std::chrono::steady_clock::now();
      if (n_odo == 0) t_first = t_last;
      ++n_odo;
      if ((want_kf || !kf_cloud_prefix.empty() || !places_path.empty()) && n_odo % (size_t)kf_every == 0) rebvio.requestKeyframe();
    });
    std::FILE *kf_pose_file = nullptr, *kf_fuse_file = nullptr, *kf_window_file = nullptr, *kf_handover_file = nullptr;
    size_t n_poses = 0, n_fusions = 0, n_window = 0, n_handovers = 0;
    if (want_kf) {
      for (auto pf : {std::make_pair(&kf_pose_path, &kf_pose_file), std::make_pair(&kf_fuse_path, &kf_fuse_file),
                      std::make_pair(&kf_window_path, &kf_window_file), std::make_pair(&kf_handover_path, &kf_handover_file)}) {
        if (pf.first->empty()) continue;
        *pf.second = std::fopen(pf.first->c_str(), "w");
        if (!*pf.second) {
          std::fprintf(stderr, "error: cannot write %s\n", pf.first->c_str());
          return 1;
        }
      }
      rebvio.registerKeyframePoseCallback([&](uint64_t ts_us, const rebvio::types::KfPose& p) {
        ++n_poses;
        if (!kf_pose_file) return;  // (--kf-fuse alone: the callback is what makes the thread align)
        std::fprintf(kf_pose_file, "%llu %d %d", (unsigned long long)ts_us, p.status, p.used);
        for (double v : p.R) std::fprintf(kf_pose_file, " %.17g", v);
        for (double v : p.t) std::fprintf(kf_pose_file, " %.17g", v);
        std::fprintf(kf_pose_file, "\n");
      });
      if (kf_fuse_file) {
        rebvio.registerKeyframeFuseCallback([&](uint64_t ts_us, const rebvio::types::KfFuse& f) {
          std::fprintf(kf_fuse_file, "%llu %d %d %d %d %d %d\n", (unsigned long long)ts_us, f.candidates, f.associated, f.fused, f.gated, f.flat,
                       f.clamped);
          ++n_fusions;
        });
        rebvio.setKeyframeDepthFusion(true);
      }
      if (kf_handover_file) {
        rebvio.registerKeyframeHandoverCallback([&](uint64_t ts_us, uint64_t kf_ts_us, const rebvio::types::KfHandover& h) {
          std::fprintf(kf_handover_file, "%llu %llu %d %d %d %d %d %d %d\n", (unsigned long long)ts_us, (unsigned long long)kf_ts_us, h.candidates,
                       h.associated, h.out_of_range, h.claimed, h.adopted, h.kept, h.conflicts);
          ++n_handovers;
        });
        rebvio.setKeyframeDepthHandover(true);
      }
      if (kf_window_file) {
        rebvio.registerKeyframeWindowCallback([&](uint64_t ts_us, const std::vector<rebvio::types::KfWindowPose>& w) {
          for (const rebvio::types::KfWindowPose& e : w) {
            std::fprintf(kf_window_file, "%llu %llu %d %d %d", (unsigned long long)ts_us, (unsigned long long)e.kf_ts_us, e.pose.status, e.pose.used,
                         e.inliers);
            for (double v : e.pose.R) std::fprintf(kf_window_file, " %.17g", v);
            for (double v : e.pose.t) std::fprintf(kf_window_file, " %.17g", v);
            std::fprintf(kf_window_file, "\n");
            ++n_window;
          }
        });
        rebvio.setKeyframeWindow(kf_window);
      }
      rebvio.setKeyframeAlign(kf_align);
      rebvio.requestKeyframe();
    }
    size_t n_kf_clouds = 0, n_kf_points = 0;
    if (!kf_cloud_prefix.empty()) {
      rebvio.registerKeyframeCloudCallback([&](const rebvio::types::PointCloud& pc) {
        rebvio::io::writePointCloudPly(kf_cloud_prefix + std::to_string(pc.ts_us) + ".ply", pc.points, pc.size, pc.ts_us);
        ++n_kf_clouds;
        n_kf_points += pc.size;
      });
      if (!want_kf) rebvio.requestKeyframe();
    }
    std::FILE* places_file = nullptr;
    if (!places_path.empty()) {
      places_file = std::fopen(places_path.c_str(), "w");
      if (!places_file) {
        std::fprintf(stderr, "error: cannot write %s\n", places_path.c_str());
        return 1;
      }
      rebvio.setPlaceRecognition(4096, 4, place_exclude);
      rebvio.registerPlaceCallback([&](uint64_t ts_us, const std::vector<rebvio::types::PlaceMatch>& matches) {
        for (const rebvio::types::PlaceMatch& m : matches)
          std::fprintf(places_file, "%llu %llu %u %d\n", (unsigned long long)ts_us, (unsigned long long)m.tag, m.distance, m.index);
      });
      if (!want_kf && kf_cloud_prefix.empty()) rebvio.requestKeyframe();
    }
    size_t n_clouds = 0, n_points = 0;
    if (!cloud_prefix.empty() || cloud_dry)
      rebvio.registerPointCloudCallback([&](const rebvio::types::PointCloud& pc) {
        if (!cloud_prefix.empty()) rebvio::io::writePointCloudPly(cloud_prefix + std::to_string(pc.ts_us) + ".ply", pc.points, pc.size, pc.ts_us);
        ++n_clouds;
        n_points += pc.size;
      });
    size_t n_polyline_files = 0, n_lines = 0, n_line_points = 0;
    if (!polylines_prefix.empty()) {
      rebvio::types::PolylineOpts po;
      po.min_chain_length = min_chain;
      rebvio.registerEdgePolylineCallback([&](const rebvio::types::EdgePolylines& ep) {
        rebvio::io::writePolylinesPly(polylines_prefix + std::to_string(ep.ts_us) + ".ply", ep.points, ep.size, ep.lines, ep.num_lines, ep.ts_us);
        ++n_polyline_files;
        n_lines += ep.num_lines;
        n_line_points += ep.size;
      }, po);
    }
    size_t n_segment_files = 0, n_segments = 0, n_segments_valid = 0;
    if (!segments_prefix.empty()) {
      rebvio::types::SegmentOpts so;
      so.poly.min_chain_length = min_chain;
      so.tol = (float)seg_tol;
      rebvio.registerEdgeSegmentCallback([&](const rebvio::types::EdgeSegments& es) {
        rebvio::io::writeSegmentsPly(segments_prefix + std::to_string(es.ts_us) + ".ply", es.segments, es.size, es.ts_us);
        ++n_segment_files;
        n_segments += es.size;
        n_segments_valid += (size_t)es.counts.depth_valid;
      }, so);
    }
    std::FILE* depth_file = nullptr;
    size_t n_depth = 0, n_depth_fused = 0, n_depth_handed = 0;
    std::vector<uint16_t> depth_frame;
    if (!depth_path.empty()) {
      depth_file = std::fopen(depth_path.c_str(), "rb");
      if (!depth_file || std::fseek(depth_file, (long)(first * (size_t)W * H * 2), SEEK_SET) != 0) {
        std::fprintf(stderr, "error: cannot read %s\n", depth_path.c_str());
        return 1;
      }
      depth_frame.resize((size_t)W * H);
      rebvio.registerDepthPriorCallback([&](uint64_t, const rebvio::types::DepthPriorCounts& c) {
        ++n_depth;
        n_depth_fused += (size_t)c.fused;
      });
    }
    std::unique_ptr<rebvio::io::StreamSource> right_src;
    size_t n_right = 0, n_right_fused = 0, n_right_handed = 0;
    if (!right_path.empty()) {
      if (!asl.empty()) right_src.reset(new rebvio::io::EurocReader(right_path, "cam1", "imu0", colour));
      else right_src.reset(new rebvio::io::RawReader(right_path, H, W, 0, dt, ""));
      if (right_src->numFrames() == 0) {
        std::fprintf(stderr, "error: cannot read %s\n", right_path.c_str());
        return 1;
      }
      rebvio::types::StereoPriorOpts so;
      so.baseline = baseline;
      rebvio.setStereo(so);
      rebvio.registerStereoPriorCallback([&](uint64_t, const rebvio::types::StereoPriorCounts& c) {
        ++n_right;
        n_right_fused += (size_t)c.fused;
      });
    }
    size_t frame_index = first;
    const size_t n = rebvio::io::replay(
        *src,
        [&](rebvio::types::Image&& im) {
          if (right_src && frame_index < right_src->numFrames()) {
            while (n_right_handed >= (size_t)rebvio.framesProcessed() + 7 && rebvio.running()) std::this_thread::sleep_for(std::chrono::microseconds(100));
            rebvio::types::Image r;
            r.ts_us = im.ts_us;
            r.data = right_src->frame(frame_index);
            rebvio.rightImageCallback(std::move(r));
            ++n_right_handed;
          }
          ++frame_index;
          if (depth_file && std::fread(depth_frame.data(), 2, depth_frame.size(), depth_file) == depth_frame.size()) {
            while (n_depth_handed >= (size_t)rebvio.framesProcessed() + 7 && rebvio.running()) std::this_thread::sleep_for(std::chrono::microseconds(100));
            rebvio::types::DepthImage d;
            d.data = depth_frame.data();
            d.rows = H;
            d.cols = W;
            d.format = rebvio::types::DEPTH_U16;
            d.unit = depth_unit;
            d.ts_us = im.ts_us;
            rebvio.depthImageCallback(std::move(d));
            ++n_depth_handed;
          }
          rebvio.imageCallback(std::move(im));
        },
        [&](rebvio::types::Imu&& s) { rebvio.imuCallback(std::move(s)); }, first, count);
    rebvio.waitIdle();
    std::fprintf(stderr, "frames=%zu odometry=%zu running=%d\n", n, n_odo, (int)rebvio.running());
    if (depth_file) {
      std::fclose(depth_file);
      std::fprintf(stderr, "depth_images=%zu depth_fused_frames=%zu depth_fused_keylines=%zu depth_dropped=%u\n", n_depth_handed, n_depth, n_depth_fused,
                   rebvio.depthImagesDropped());
    }
    if (right_src)
      std::fprintf(stderr, "right_images=%zu stereo_fused_frames=%zu stereo_fused_keylines=%zu right_dropped=%u\n", n_right_handed, n_right, n_right_fused,
                   rebvio.rightImagesDropped());
    if (places_file) {
      std::fclose(places_file);
      std::fprintf(stderr, "place_queries=%u place_matches=%u place_misses=%u\n", rebvio.placeQueries(), rebvio.placeMatches(), rebvio.placeMisses());
    }
    if (!cloud_prefix.empty() || cloud_dry) std::fprintf(stderr, "clouds=%zu points=%zu\n", n_clouds, n_points);
    if (!kf_cloud_prefix.empty()) std::fprintf(stderr, "kf_clouds=%zu kf_points=%zu\n", n_kf_clouds, n_kf_points);
    if (!polylines_prefix.empty()) std::fprintf(stderr, "polyline_files=%zu lines=%zu line_points=%zu\n", n_polyline_files, n_lines, n_line_points);
    if (!segments_prefix.empty()) std::fprintf(stderr, "segment_files=%zu segments=%zu segments_valid=%zu\n", n_segment_files, n_segments, n_segments_valid);
    if (kf_pose_file) std::fclose(kf_pose_file);
    if (want_kf) std::fprintf(stderr, "kf_poses=%zu\n", n_poses);
    if (kf_window_file) {
      std::fclose(kf_window_file);
      std::fprintf(stderr, "kf_window_lines=%zu\n", n_window);
    }
    if (kf_fuse_file) {
      std::fclose(kf_fuse_file);
      std::fprintf(stderr, "kf_fusions=%zu\n", n_fusions);
    }
    if (kf_handover_file) {
      std::fclose(kf_handover_file);
      std::fprintf(stderr, "kf_handovers=%zu\n", n_handovers);
    }
    if (n_odo > 1) {  // wall clock between the first and the last published odometry: the whole class, input thread included
      const double sec = std::chrono::duration<double>(t_last - t_first).count();
      std::fprintf(stderr, "[replay] %zu odometry records in %.3f s = %.0f frames/s (wall clock, first to last record)\n", n_odo, sec,
                   (double)(n_odo - 1) / sec);
    }
    return (n_odo + 1 == n || n == 0) ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
