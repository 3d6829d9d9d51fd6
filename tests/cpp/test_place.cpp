// rebvio::EdgeMap::placeSignature, rebvio::PlaceDb and rebvio::Rebvio::setPlaceRecognition / registerPlaceCallback on a synthetic
// ping-pong stream (GPU): the camera goes out over <base> frames and comes back over the same ones.
//   test_place <frames.u8> <W> <H> <N> <base> <fm> <cx> <cy> <keylines_ref> <keylines_max> <min matches> <every> <exclude_last>
// The classes: a detected map's signature sums to 65535 within the rounding of 384 words and counts every keyline; a database
// finds the map it was given at distance 0, moves, refuses nothing it should take and returns -1 when full.
// The pipeline: the stream twice, with the same keyframe requests - in front of every <every>-th frame, handed in once the tracker
// has caught up, so that the way back marks the frames the way out marked - once without and once with place recognition
// (exclude_last as given, every match handed out). The odometry lines are byte-identical. Every mark calls the callback once, with
// the record's stamp. The marks are read from the stamps: for every mark on the way back for which an eligible entry lies within
// 2 base frames, the best match's tag is a keyframe within 2 base frames of the query's own and its distance is below half the
// runner-up's. Tags are the stamps of earlier marks, indices their order, distances ascend.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

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
  std::string frames;
  int W, H, N, base, kref, kmax, min_matches, every, exclude_last;
  float fm, cx, cy;
};

struct Mark {
  uint64_t ts;
  std::vector<rebvio::types::PlaceMatch> matches;
};
struct Run {
  std::vector<std::string> lines;
  std::vector<Mark> marks;
  unsigned queries = 0, matches = 0, misses = 0;
  bool running = false;
};

// the base frame shown at stream position j (synth.pingpong_indices)
static int base_of(const Args& a, int j) {
  const int period = 2 * a.base - 2;
  const int k = j % period;
  return k < a.base ? k : period - k;
}

static Run run(const Args& a, bool places, int capacity) {
  Run out;
  rebvio::RebvioConfig config;
  config.camera = rebvio::Camera(a.H, a.W, a.fm, a.fm, a.cx, a.cy);
  config.edge_detector.keylines_ref = a.kref;
  config.edge_detector.keylines_max = a.kmax;
  config.core.global_min_matches_threshold = (unsigned)a.min_matches;
  rebvio::io::RawReader src(a.frames, a.H, a.W, 0, 50000);
  rebvio::Rebvio rebvio(config);
  std::mutex mu;
  rebvio.registerOdometryCallback([&](rebvio::types::Odometry& o) {
    std::lock_guard<std::mutex> g(mu);
    out.lines.push_back(rebvio::io::OdometryWriter::format(o));
  });
  if (places) {
    rebvio.setPlaceRecognition(capacity, 4, a.exclude_last, rebvio::types::kPlaceMaxDistance);
    rebvio.registerPlaceCallback([&](uint64_t ts_us, const std::vector<rebvio::types::PlaceMatch>& m) {
      std::lock_guard<std::mutex> g(mu);
      out.marks.push_back(Mark{ts_us, m});
    });
  }
  int handed = 0;
  rebvio::io::replay(
      src,
      [&](rebvio::types::Image&& im) {
        if (handed >= a.every && handed % a.every == 0) {
          // the tracker has caught up: the request is seen by the pair that ends at this frame
          while ((int)rebvio.framesProcessed() < handed - 1 && rebvio.running()) std::this_thread::sleep_for(std::chrono::microseconds(100));
          rebvio.requestKeyframe();
        }
        ++handed;
        rebvio.imageCallback(std::move(im));
      },
      [&](rebvio::types::Imu&& s) { rebvio.imuCallback(std::move(s)); });
  rebvio.waitIdle();
  out.running = rebvio.running();
  out.queries = rebvio.placeQueries();
  out.matches = rebvio.placeMatches();
  out.misses = rebvio.placeMisses();
  return out;
}

int main(int argc, char** argv) {
  if (argc < 14) return 2;
  Args a;
  a.frames = argv[1];
  a.W = std::atoi(argv[2]); a.H = std::atoi(argv[3]); a.N = std::atoi(argv[4]); a.base = std::atoi(argv[5]);
  a.fm = (float)std::atof(argv[6]); a.cx = (float)std::atof(argv[7]); a.cy = (float)std::atof(argv[8]);
  a.kref = std::atoi(argv[9]); a.kmax = std::atoi(argv[10]);
  a.min_matches = std::atoi(argv[11]);
  a.every = std::atoi(argv[12]); a.exclude_last = std::atoi(argv[13]);
  try {
    // ---- the classes --------------------------------------------------------------------------------------------------------------
    {
      auto cam = std::make_shared<rebvio::Camera>(a.H, a.W, a.fm, a.fm, a.cx, a.cy);
      auto dcfg = std::make_shared<rebvio::EdgeDetectorConfig>();
      dcfg->keylines_ref = a.kref;
      dcfg->keylines_max = a.kmax;
      rebvio::EdgeDetector detector(cam, dcfg);
      rebvio::io::RawReader src(a.frames, a.H, a.W, 0, 50000);
      rebvio::types::Image i0{0, src.frame(0)}, i1{50000, src.frame(9)};
      rebvio::EdgeMap::SharedPtr m0 = detector.detect(i0), m1 = detector.detect(i1);
      int c0 = -1, c1 = -1;
      const rebvio::types::PlaceSignature s0 = m0->placeSignature(&c0), s1 = m1->placeSignature(&c1);
      long sum = 0;
      for (uint16_t w : s0) sum += w;
      CHECK(c0 == m0->size() && c1 == m1->size() && c0 > 100);
      CHECK(sum > 65535 - rebvio::types::kPlaceWords && sum <= 65535);
      CHECK(s0 != s1 && m0->placeSignature() == s0);
      rebvio::PlaceDb db = m0->placeDb(2);
      CHECK(db && db.size() == 0 && db.capacity() == 2 && db.query(*m0, 4).empty());
      CHECK(db.add(*m0, 111) == 0 && db.add(*m1, 222) == 1 && db.size() == 2);
      CHECK(db.add(*m1, 333) == -1 && db.addSignature(s0, c0, 444) == -1 && db.size() == 2);  // full
      int counted = -1;
      uint64_t tag = 0;
      CHECK(db.entry(1, &counted, &tag) == s1 && counted == c1 && tag == 222);
      std::vector<rebvio::types::PlaceMatch> got = db.query(*m1, 4);
      CHECK(got.size() == 2 && got[0].distance == 0 && got[0].index == 1 && got[0].tag == 222 && got[1].index == 0 && got[1].tag == 111 &&
            got[1].distance > 0);
      CHECK(db.query(*m1, 4, 1).size() == 1 && db.query(*m1, 4, 2).empty());
      const std::vector<rebvio::types::PlaceMatch> again = db.querySignature(s1, 1);
      CHECK(again.size() == 1 && again[0].distance == 0 && again[0].index == 1);
      rebvio::PlaceDb moved = std::move(db);
      CHECK(!db && moved && moved.size() == 2);
      moved.clear();
      CHECK(moved.size() == 0 && moved.addSignature(s0, c0, 555) == 0 && moved.entry(0) == s0);
      bool refused = false;
      try {
        moved.query(*m0, 17);
      } catch (const std::exception&) {
        refused = true;
      }
      CHECK(refused);
      moved.reset();
      CHECK(!moved);
    }
    // ---- the pipeline -------------------------------------------------------------------------------------------------------------
    const Run off = run(a, false, 0), on = run(a, true, 64), tiny = run(a, true, 3);
    CHECK(off.running && on.running && tiny.running);
    CHECK((int)off.lines.size() == a.N - 1 && off.lines == on.lines && off.lines == tiny.lines);
    CHECK(off.marks.empty() && off.queries == 0);
    const int want_marks = (a.N - 1) / a.every;
    CHECK((int)on.marks.size() == want_marks && on.queries == on.marks.size() && on.misses == 0);
    CHECK((int)tiny.marks.size() == want_marks && tiny.misses == (unsigned)(want_marks - 3));  // a full database stops adding, and counts
    size_t total = 0;
    int checked = 0;
    for (size_t q = 0; q < on.marks.size(); ++q) {
      const Mark& m = on.marks[q];
      total += m.matches.size();
      CHECK(m.ts % 50000 == 0 && (q == 0 || m.ts > on.marks[q - 1].ts));
      const int jq = (int)(m.ts / 50000), bq = base_of(a, jq);
      const int eligible = (int)q - a.exclude_last > 0 ? (int)q - a.exclude_last : 0;
      CHECK((int)m.matches.size() == (eligible < 4 ? eligible : 4));
      for (size_t r = 0; r < m.matches.size(); ++r) {
        const rebvio::types::PlaceMatch& x = m.matches[r];
        CHECK(x.index >= 0 && x.index < eligible && x.tag == on.marks[(size_t)x.index].ts);
        if (r > 0) CHECK(m.matches[r - 1].distance < x.distance || (m.matches[r - 1].distance == x.distance && m.matches[r - 1].index < x.index));
      }
      bool counterpart = false;
      for (int e = 0; e < eligible; ++e) counterpart = counterpart || std::abs(base_of(a, (int)(on.marks[(size_t)e].ts / 50000)) - bq) <= 2;
      std::printf("mark %zu: frame %d (base %d)%s", q, jq, bq, counterpart ? " *" : "");
      for (const rebvio::types::PlaceMatch& x : m.matches) std::printf("  [%d: frame %d, d %u]", x.index, (int)(x.tag / 50000), x.distance);
      std::printf("\n");
      if (jq < a.base || !counterpart) continue;
      ++checked;
      CHECK(!m.matches.empty());
      if (m.matches.empty()) continue;
      CHECK(std::abs(base_of(a, (int)(m.matches[0].tag / 50000)) - bq) <= 2);
      if (m.matches.size() > 1) CHECK(2ull * m.matches[0].distance < m.matches[1].distance);
    }
    CHECK(checked >= 3 && total == on.matches);
    for (size_t q = 0; q < tiny.marks.size(); ++q)  // the first three marks are all it ever holds
      for (const rebvio::types::PlaceMatch& x : tiny.marks[q].matches) CHECK(x.index < 3 - a.exclude_last);
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
