// rebvio::EdgeMap::edgeSegments, rebvio::Rebvio::registerEdgeSegmentCallback and io::writeSegmentsPly / readSegmentsPly on a synthetic
// stream (GPU).
//   test_edge_segments <frames.u8> <W> <H> <N> <fm> <cx> <cy> <keylines_ref> <keylines_max> <imu.bin> <min matches> <tmp dir>
// The classes: the segments of a detected map (an open filter: a fresh map carries no depth yet) against the map's polylines under
// the same options - every segment lies inside one line, adjacent segments of a line share their vertex, the end points are the
// pos_img of the polyline points' keylines and, where the depth is valid, lie on the ray of that keyline; the counts; a refusal.
// The callback: the stream three times - no callback, a segment callback beside a polyline callback, a polyline callback alone. The
// odometry lines of all three are byte-identical; the segment callback is called once per record, behind the polyline callback, with
// its stamp and pose; first_point / points index that record's polyline points.
// The PLY round trip: two vertices and one edge per depth-valid segment; the readers take their own files only.
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
  std::string frames, imu, tmp;
  int W, H, N, kref, kmax, min_matches;
  float fm, cx, cy;
};

struct PolyRec {
  uint64_t ts;
  rebvio::types::CloudPose pose;
  std::vector<rebvio::types::CloudPoint> points;
  std::vector<rebvio::types::Polyline> lines;
  size_t order;  // position among the record's callbacks
};
struct SegRec {
  uint64_t ts;
  rebvio::types::CloudPose pose;
  std::vector<rebvio::types::LineSegment> segs;
  rebvio::types::SegmentCounts counts;
  size_t order;
};
struct Run {
  std::vector<std::string> lines;
  std::vector<PolyRec> polys;
  std::vector<SegRec> segs;
  bool running = false;
};

static Run run(const Args& a, bool poly_cb, bool seg_cb) {
  Run out;
  rebvio::RebvioConfig config;
  config.camera = rebvio::Camera(a.H, a.W, a.fm, a.fm, a.cx, a.cy);
  config.edge_detector.keylines_ref = a.kref;
  config.edge_detector.keylines_max = a.kmax;
  config.core.global_min_matches_threshold = (unsigned)a.min_matches;
  rebvio::io::RawReader src(a.frames, a.H, a.W, 0, 50000, a.imu);
  rebvio::Rebvio rebvio(config);
  std::mutex mu;
  size_t calls = 0;
  rebvio.registerOdometryCallback([&](rebvio::types::Odometry& o) {
    std::lock_guard<std::mutex> g(mu);
    out.lines.push_back(rebvio::io::OdometryWriter::format(o));
  });
  rebvio::types::SegmentOpts so;
  so.poly.min_chain_length = 4;
  so.min_points = 4;
  if (seg_cb)  // registered first: it is still called behind the polyline callback
    rebvio.registerEdgeSegmentCallback([&](const rebvio::types::EdgeSegments& es) {
      std::lock_guard<std::mutex> g(mu);
      out.segs.push_back(SegRec{es.ts_us, es.pose, std::vector<rebvio::types::LineSegment>(es.segments, es.segments + es.size), es.counts, calls++});
    }, so);
  if (poly_cb)
    rebvio.registerEdgePolylineCallback([&](const rebvio::types::EdgePolylines& ep) {
      std::lock_guard<std::mutex> g(mu);
      out.polys.push_back(PolyRec{ep.ts_us, ep.pose, std::vector<rebvio::types::CloudPoint>(ep.points, ep.points + ep.size),
                                  std::vector<rebvio::types::Polyline>(ep.lines, ep.lines + ep.num_lines), calls++});
    }, so.poly);
  rebvio::io::replay(src, [&](rebvio::types::Image&& im) { rebvio.imageCallback(std::move(im)); },
                     [&](rebvio::types::Imu&& s) { rebvio.imuCallback(std::move(s)); });
  rebvio.waitIdle();
  out.running = rebvio.running();
  return out;
}

// every segment inside one line of the polylines, in order, adjacent ones of a line sharing their vertex; returns the depth-valid ones
static size_t check_against_lines(const std::vector<rebvio::types::LineSegment>& segs, const rebvio::types::SegmentCounts& cnt,
                                  const std::vector<rebvio::types::CloudPoint>& points, const std::vector<rebvio::types::Polyline>& lines,
                                  const rebvio::types::SegmentOpts& so) {
  CHECK((size_t)cnt.kept == segs.size() && (size_t)cnt.points == points.size() && (size_t)cnt.lines == lines.size());
  CHECK(cnt.segments_all >= cnt.kept && cnt.depth_valid <= cnt.kept && cnt.rounds_used >= 0 && cnt.rounds_used <= so.max_rounds);
  size_t valid = 0;
  int prev_end = -1, prev_line = -1;
  for (const rebvio::types::LineSegment& s : segs) {
    CHECK(s.line >= 0 && (size_t)s.line < lines.size() && s.points >= so.min_points && (s.flags & ~3) == 0);
    if (s.line < 0 || (size_t)s.line >= lines.size()) continue;
    const rebvio::types::Polyline& l = lines[(size_t)s.line];
    const int last = s.first_point + s.points - 1;
    CHECK(s.first_point >= l.first_point && last < l.first_point + l.points);
    CHECK(s.line > prev_line || (s.line == prev_line && s.first_point >= prev_end));  // in point order; neighbours share at most a vertex
    prev_line = s.line;
    prev_end = last;
    const float dx = s.uv1[0] - s.uv0[0], dy = s.uv1[1] - s.uv0[1];
    CHECK(dx * dx + dy * dy >= so.min_length * so.min_length && s.max_dev2 >= 0.0f);
    if (!(s.flags & 2)) CHECK(s.max_dev2 <= so.tol * so.tol);
    if (s.flags & 1) {
      ++valid;
      CHECK(s.rho0 > 0.0f && s.rho1 > 0.0f && s.sigma_rho0 >= 0.0f && s.sigma_rho1 >= 0.0f && s.chi2 >= 0.0f);
    } else {
      CHECK(s.rho0 == 0.0f && s.rho1 == 0.0f && s.xyz0[2] == 0.0f && s.xyz1[2] == 0.0f);
    }
  }
  CHECK(valid == (size_t)cnt.depth_valid);
  return valid;
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
  a.tmp = argv[12];
  try {
    // ---- the classes ------------------------------------------------------------------------------------------------------------
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
      const std::vector<rebvio::types::KeyLine>& kl = map->keylines();
      rebvio::types::SegmentOpts so;
      so.poly.filter = rebvio::types::CloudFilter{0, 1e9f, 1e-3f, 20.0f};
      rebvio::types::CloudPose pose;
      pose.t[0] = 0.25f; pose.t[2] = -1.0f; pose.scale = 2.0f;
      const rebvio::EdgeMap::EdgeSegments sg = map->edgeSegments(so, pose);
      const rebvio::EdgeMap::EdgePolylines pl = map->edgePolylines(so.poly, pose);
      const size_t valid = check_against_lines(sg.segments, sg.counts, pl.points, pl.lines, so);
      std::printf("classes: %d keylines, %zu points in %zu lines, %d segments, %zu kept, %zu with a depth, %d rounds\n", map->size(), pl.points.size(),
                  pl.lines.size(), sg.counts.segments_all, sg.segments.size(), valid, sg.counts.rounds_used);
      CHECK(sg.segments.size() > 20 && valid > 20 && sg.counts.unresolved == 0 && sg.counts.rounds_used >= 3);
      for (const rebvio::types::LineSegment& s : sg.segments) {
        const rebvio::types::CloudPoint& p0 = pl.points[(size_t)s.first_point];
        const rebvio::types::CloudPoint& p1 = pl.points[(size_t)(s.first_point + s.points - 1)];
        const rebvio::types::KeyLine &k0 = kl[(size_t)p0.keyline], &k1 = kl[(size_t)p1.keyline];
        CHECK(s.uv0[0] == k0.pos_img[0] && s.uv0[1] == k0.pos_img[1] && s.uv1[0] == k1.pos_img[0] && s.uv1[1] == k1.pos_img[1]);
        if (!(s.flags & 1)) continue;
        // detection leaves rho = 1 everywhere: the fitted ends are 1 and the end points are the polyline's own points
        CHECK(std::fabs(s.rho0 - 1.0f) < 1e-5f && std::fabs(s.rho1 - 1.0f) < 1e-5f);
        for (int k = 0; k < 3; ++k) CHECK(std::fabs(s.xyz0[k] - p0.xyz[k]) < 1e-4f && std::fabs(s.xyz1[k] - p1.xyz[k]) < 1e-4f);
      }
      rebvio::types::SegmentOpts bad;
      bad.max_rounds = 0;
      bool refused = false;
      try {
        map->edgeSegments(bad);
      } catch (const std::exception&) {
        refused = true;
      }
      CHECK(refused);

      // ---- the PLY round trip ---------------------------------------------------------------------------------------------------
      std::vector<rebvio::types::LineSegment> mixed(sg.segments.begin(), sg.segments.begin() + 10);
      mixed[3].flags = 0;  // a segment without a depth is left out
      mixed[7].flags = 2;
      const std::string path = a.tmp + "/segments.ply";
      rebvio::io::writeSegmentsPly(path, mixed.data(), mixed.size(), 123456789ull);
      std::vector<rebvio::io::PlyEdge> edges;
      uint64_t ts = 0;
      const std::vector<rebvio::io::PlyVertex> v = rebvio::io::readSegmentsPly(path, &edges, &ts);
      CHECK(ts == 123456789ull && v.size() == 16 && edges.size() == 8);
      size_t e = 0;
      for (size_t i = 0; i < mixed.size(); ++i) {
        if (!(mixed[i].flags & 1)) continue;
        CHECK(e < edges.size() && edges[e].vertex1 == (int)(2 * e) && edges[e].vertex2 == (int)(2 * e + 1));
        CHECK(std::memcmp(&v[2 * e].x, mixed[i].xyz0, 12) == 0 && std::memcmp(&v[2 * e + 1].x, mixed[i].xyz1, 12) == 0);
        CHECK(v[2 * e].intensity == mixed[i].sigma_rho0 && v[2 * e + 1].intensity == mixed[i].sigma_rho1);
        ++e;
      }
      CHECK(e == 8);
      rebvio::io::writeSegmentsPly(path, nullptr, 0, 1);
      CHECK(rebvio::io::readSegmentsPly(path, &edges, &ts).empty() && edges.empty() && ts == 1);
      refused = false;  // the readers take their own files only
      try {
        rebvio::io::readPolylinesPly(path, &edges);
      } catch (const std::exception&) {
        refused = true;
      }
      CHECK(refused);
      rebvio::io::writePolylinesPly(path, pl.points.data(), 5, pl.lines.data(), 1, 3);
      refused = false;
      try {
        rebvio::io::readSegmentsPly(path, &edges);
      } catch (const std::exception&) {
        refused = true;
      }
      CHECK(refused);
    }

    // ---- the callback -------------------------------------------------------------------------------------------------------------
    const Run plain = run(a, false, false), both = run(a, true, true), poly_only = run(a, true, false);
    for (const Run* r : {&plain, &both, &poly_only}) {
      CHECK(r->running);
      CHECK(r->lines == plain.lines);
    }
    CHECK((int)plain.lines.size() == a.N - 1 && plain.segs.empty() && poly_only.segs.empty() && plain.polys.empty());
    CHECK(both.segs.size() == plain.lines.size() && both.polys.size() == both.segs.size() && poly_only.polys.size() == both.polys.size());
    rebvio::types::SegmentOpts so;
    so.poly.min_chain_length = 4;
    so.min_points = 4;
    size_t total = 0, total_valid = 0;
    for (size_t i = 0; i < both.segs.size() && i < both.polys.size(); ++i) {
      const SegRec& s = both.segs[i];
      const PolyRec& p = both.polys[i];
      CHECK(s.ts == p.ts && s.ts == (uint64_t)(i + 1) * 50000ull && std::memcmp(&s.pose, &p.pose, sizeof(s.pose)) == 0);
      CHECK(p.order == 2 * i && s.order == 2 * i + 1);  // the polyline callback of a record first
      if (i < poly_only.polys.size())  // the polylines are what they are without the segment callback
        CHECK(p.points.size() == poly_only.polys[i].points.size() &&
              (p.points.empty() || std::memcmp(p.points.data(), poly_only.polys[i].points.data(), p.points.size() * sizeof(rebvio::types::CloudPoint)) == 0));
      total_valid += check_against_lines(s.segs, s.counts, p.points, p.lines, so);
      total += s.segs.size();
      for (const rebvio::types::LineSegment& g : s.segs) {
        if (!(g.flags & 1)) continue;
        // the end point lies on the ray of the polyline point it begins at: xyz - t is parallel to that point's xyz - t
        const rebvio::types::CloudPoint& p0 = p.points[(size_t)g.first_point];
        float va[3], vb[3];
        for (int k = 0; k < 3; ++k) { va[k] = g.xyz0[k] - s.pose.t[k]; vb[k] = p0.xyz[k] - s.pose.t[k]; }
        const float cx = va[1] * vb[2] - va[2] * vb[1], cy = va[2] * vb[0] - va[0] * vb[2], cz = va[0] * vb[1] - va[1] * vb[0];
        const float na = std::sqrt(va[0] * va[0] + va[1] * va[1] + va[2] * va[2]), nb = std::sqrt(vb[0] * vb[0] + vb[1] * vb[1] + vb[2] * vb[2]);
        CHECK(std::sqrt(cx * cx + cy * cy + cz * cz) <= 1e-4f * na * nb);
      }
    }
    std::printf("callback: %zu records, %zu segments, %zu with a depth\n", both.segs.size(), total, total_valid);
    CHECK(total > 10 && total_valid > 5);
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    ++fails;
  }
  if (fails == 0) std::printf("ok\n");
  return fails ? 1 : 0;
}
