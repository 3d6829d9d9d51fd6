// rebvio::EdgeMap::edgeChains / edgePolylines, rebvio::Rebvio::registerEdgePolylineCallback and io::writePolylinesPly / readPolylinesPly
// on a synthetic stream (GPU).
//   test_edge_polylines <frames.u8> <W> <H> <N> <fm> <cx> <cy> <keylines_ref> <keylines_max> <imu.bin> <min matches> <tmp dir>
// The classes: the chains of a detected map against a walk of succ over the map's own keylines (EdgeMap::keylines), the table's
// identities; the polylines with an open filter against the map's cloud, record by record.
// The callback: the stream three times - no callback, a polyline callback beside a point-cloud callback, and a point-cloud callback
// alone. The odometry lines of all three are byte-identical; the polyline callback is called once per record with the record's stamp
// and the pose of the point-cloud callback of the same record; every point is the bytes of the cloud's record of the same keyline;
// lines are runs of consecutive ranks.
// The PLY round trip: vertices, edges per consecutive pair, the closing edge of a closed line, a cut at a cap; refusals.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
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
  std::vector<int> refs;
  std::vector<rebvio::types::Polyline> lines;
};
struct CloudRec {
  uint64_t ts;
  rebvio::types::CloudPose pose;
  std::vector<rebvio::types::CloudPoint> points;
};
struct Run {
  std::vector<std::string> lines;
  std::vector<PolyRec> polys;
  std::vector<CloudRec> clouds;
  bool running = false;
};

static Run run(const Args& a, bool poly_cb, bool cloud_cb, int min_chain) {
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
  });
  if (cloud_cb)
    rebvio.registerPointCloudCallback([&](const rebvio::types::PointCloud& pc) {
      std::lock_guard<std::mutex> g(mu);
      out.clouds.push_back(CloudRec{pc.ts_us, pc.pose, std::vector<rebvio::types::CloudPoint>(pc.points, pc.points + pc.size)});
    });
  if (poly_cb) {
    rebvio::types::PolylineOpts po;
    po.min_chain_length = min_chain;
    rebvio.registerEdgePolylineCallback([&](const rebvio::types::EdgePolylines& ep) {
      std::lock_guard<std::mutex> g(mu);
      out.polys.push_back(PolyRec{ep.ts_us, ep.pose, std::vector<rebvio::types::CloudPoint>(ep.points, ep.points + ep.size),
                                  std::vector<int>(ep.refs, ep.refs + 2 * ep.size),
                                  std::vector<rebvio::types::Polyline>(ep.lines, ep.lines + ep.num_lines)});
    }, po);
  }
  rebvio::io::replay(src, [&](rebvio::types::Image&& im) { rebvio.imageCallback(std::move(im)); },
                     [&](rebvio::types::Imu&& s) { rebvio.imuCallback(std::move(s)); });
  rebvio.waitIdle();
  out.running = rebvio.running();
  return out;
}

// lines partition the points; ranks inside a line are consecutive; a closed line is a whole chain
static void check_lines(const std::vector<rebvio::types::Polyline>& lines, const std::vector<int>& refs, size_t n_points, int min_chain) {
  int at = 0;
  for (const rebvio::types::Polyline& l : lines) {
    CHECK(l.first_point == at && l.points >= 1 && (l.flags & ~1) == 0);
    for (int k = 0; k < l.points && (size_t)(at + k) < n_points; ++k) {
      CHECK(refs[2 * (size_t)(at + k)] == l.head);
      if (k > 0) CHECK(refs[2 * (size_t)(at + k) + 1] == refs[2 * (size_t)(at + k - 1) + 1] + 1);
    }
    if (l.flags & 1) CHECK(refs[2 * (size_t)at + 1] == 0 && l.points >= min_chain);
    at += l.points;
  }
  CHECK((size_t)at == n_points);
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
      const int n = map->size();
      CHECK(n > 100);
      const std::vector<rebvio::types::KeyLine>& kl = map->keylines();
      const rebvio::EdgeMap::EdgeChains ch = map->edgeChains();
      CHECK((int)ch.refs.size() == n && (int)ch.order.size() == n && ch.starts.size() >= 2 && ch.starts.front() == 0 && ch.starts.back() == n);
      auto succ = [&](int i) {
        const int s = kl[(size_t)i].id_next;
        return (s >= 0 && s < n && s != i && kl[(size_t)s].id_prev == i) ? s : -1;
      };
      int longest = 0, prev_head = -1;
      for (size_t c = 0; c + 1 < ch.starts.size(); ++c) {
        const int s0 = ch.starts[c], L = ch.starts[c + 1] - s0, head = ch.order[(size_t)s0];
        CHECK(L >= 1 && head > prev_head);
        prev_head = head;
        longest = L > longest ? L : longest;
        const int cyc = ch.refs[(size_t)head].flags & 1;
        for (int r = 0; r < L; ++r) {
          const int k = ch.order[(size_t)(s0 + r)];
          const rebvio::types::ChainRef& ref = ch.refs[(size_t)k];
          CHECK(ref.head == head && ref.rank == r && ref.length == L && ref.flags == cyc);
          CHECK(succ(k) == (r + 1 < L ? ch.order[(size_t)(s0 + r + 1)] : (cyc ? head : -1)));
        }
      }
      std::printf("classes: %d keylines, %zu chains, longest %d\n", n, ch.starts.size() - 1, longest);
      CHECK(longest > 50);
      // a fresh map carries no depth yet: the filter is opened for it, and every keyline of a long enough chain is a point
      rebvio::types::PolylineOpts open;
      open.filter = rebvio::types::CloudFilter{0, 1e9f, 1e-3f, 20.0f};
      rebvio::types::CloudPose pose;
      pose.t[0] = 0.25f; pose.t[2] = -1.0f; pose.scale = 2.0f;
      const rebvio::EdgeMap::EdgePolylines pl = map->edgePolylines(open, pose);
      const std::vector<rebvio::types::CloudPoint> cloud = map->pointCloud(open.filter, pose);
      CHECK((int)cloud.size() == n);
      size_t want_points = 0;
      for (int i = 0; i < n; ++i) want_points += ch.refs[(size_t)i].length >= 8;
      CHECK(pl.points.size() == want_points && pl.refs.size() == want_points && !pl.lines.empty());
      for (size_t p = 0; p < pl.points.size(); ++p) {
        const int k = pl.points[p].keyline;
        CHECK(k >= 0 && k < n && std::memcmp(&pl.points[p], &cloud[(size_t)k], sizeof(rebvio::types::CloudPoint)) == 0);
        CHECK(pl.refs[p][0] == ch.refs[(size_t)k].head && pl.refs[p][1] == ch.refs[(size_t)k].rank);
      }
      std::vector<int> flat;
      for (const auto& r : pl.refs) { flat.push_back(r[0]); flat.push_back(r[1]); }
      check_lines(pl.lines, flat, pl.points.size(), 8);
      rebvio::types::PolylineOpts bad;
      bad.min_chain_length = 0;
      bool refused = false;
      try {
        map->edgePolylines(bad);
      } catch (const std::exception&) {
        refused = true;
      }
      CHECK(refused);

      // ---- the PLY round trip ---------------------------------------------------------------------------------------------------
      const std::string path = a.tmp + "/lines.ply";
      rebvio::io::writePolylinesPly(path, pl.points.data(), pl.points.size(), pl.lines.data(), pl.lines.size(), 123456789ull);
      std::vector<rebvio::io::PlyEdge> edges;
      uint64_t ts = 0;
      const std::vector<rebvio::io::PlyVertex> v = rebvio::io::readPolylinesPly(path, &edges, &ts);
      CHECK(ts == 123456789ull && v.size() == pl.points.size());
      for (size_t p = 0; p < v.size() && p < pl.points.size(); ++p)
        CHECK(std::memcmp(&v[p].x, pl.points[p].xyz, 12) == 0 && std::memcmp(&v[p].intensity, &pl.points[p].gradient_norm, 4) == 0);
      size_t e = 0;
      for (const rebvio::types::Polyline& l : pl.lines) {
        for (int k = 0; k + 1 < l.points; ++k, ++e) CHECK(e < edges.size() && edges[e].vertex1 == l.first_point + k && edges[e].vertex2 == l.first_point + k + 1);
        if (l.flags & 1) {
          CHECK(e < edges.size() && edges[e].vertex1 == l.first_point + l.points - 1 && edges[e].vertex2 == l.first_point);
          ++e;
        }
      }
      CHECK(e == edges.size());
      // hand-made lines: an open line of 3, a closed line of 4, a single point, a line cut by the cap (and then not closed)
      const rebvio::types::Polyline hand[4] = {{0, 3, 0, 0}, {3, 4, 9, 1}, {7, 1, 20, 0}, {8, 5, 30, 1}};
      CHECK(pl.points.size() >= 10);
      rebvio::io::writePolylinesPly(path, pl.points.data(), 10, hand, 4, 7);
      const std::vector<rebvio::io::PlyVertex> v2 = rebvio::io::readPolylinesPly(path, &edges, &ts);
      const int want_e[][2] = {{0, 1}, {1, 2}, {3, 4}, {4, 5}, {5, 6}, {6, 3}, {8, 9}};
      CHECK(v2.size() == 10 && ts == 7 && edges.size() == 7);
      for (size_t k = 0; k < 7 && k < edges.size(); ++k) CHECK(edges[k].vertex1 == want_e[k][0] && edges[k].vertex2 == want_e[k][1]);
      rebvio::io::writePolylinesPly(path, nullptr, 0, nullptr, 0, 1);
      CHECK(rebvio::io::readPolylinesPly(path, &edges, &ts).empty() && edges.empty() && ts == 1);
      // the two readers take their own files only
      refused = false;
      try {
        rebvio::io::readPointCloudPly(path);
      } catch (const std::exception&) {
        refused = true;
      }
      CHECK(refused);
      rebvio::io::writePointCloudPly(path, pl.points.data(), 5, 3);
      refused = false;
      try {
        rebvio::io::readPolylinesPly(path, &edges);
      } catch (const std::exception&) {
        refused = true;
      }
      CHECK(refused);
    }

    // ---- the callback -------------------------------------------------------------------------------------------------------------
    const Run plain = run(a, false, false, 8), both = run(a, true, true, 4), cloud_only = run(a, false, true, 8);
    for (const Run* r : {&plain, &both, &cloud_only}) {
      CHECK(r->running);
      CHECK(r->lines == plain.lines);
    }
    CHECK((int)plain.lines.size() == a.N - 1 && plain.polys.empty() && cloud_only.polys.empty());
    CHECK(both.polys.size() == plain.lines.size() && both.clouds.size() == both.polys.size() && cloud_only.clouds.size() == both.clouds.size());
    size_t total_points = 0, total_lines = 0;
    for (size_t i = 0; i < both.polys.size() && i < both.clouds.size(); ++i) {
      const PolyRec& p = both.polys[i];
      const CloudRec& c = both.clouds[i];
      CHECK(p.ts == c.ts && p.ts == (uint64_t)(i + 1) * 50000ull && std::memcmp(&p.pose, &c.pose, sizeof(p.pose)) == 0);
      // the clouds are what they are without the polyline callback
      if (i < cloud_only.clouds.size())
        CHECK(c.points.size() == cloud_only.clouds[i].points.size() &&
              (c.points.empty() || std::memcmp(c.points.data(), cloud_only.clouds[i].points.data(), c.points.size() * sizeof(rebvio::types::CloudPoint)) == 0));
      std::map<int, const rebvio::types::CloudPoint*> by_keyline;
      for (const rebvio::types::CloudPoint& q : c.points) by_keyline[q.keyline] = &q;
      for (const rebvio::types::CloudPoint& q : p.points) {
        auto it = by_keyline.find(q.keyline);
        CHECK(it != by_keyline.end() && std::memcmp(it->second, &q, sizeof(q)) == 0);  // same filter, same pose: the cloud's bytes
      }
      CHECK(p.points.size() <= c.points.size());
      check_lines(p.lines, p.refs, p.points.size(), 4);
      total_points += p.points.size();
      total_lines += p.lines.size();
    }
    std::printf("callback: %zu records, %zu points in %zu lines\n", both.polys.size(), total_points, total_lines);
    CHECK(total_points > 100 && total_lines > 10);
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    ++fails;
  }
  if (fails == 0) std::printf("ok\n");
  return fails ? 1 : 0;
}
