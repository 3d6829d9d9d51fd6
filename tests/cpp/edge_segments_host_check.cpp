// The host side of rebvio_hip_map_edge_segments (rebvio_amd/csrc/edge_segments.hpp: the per-point statements and esg::segments_host
// over them - what rebvio_hip_test_edge_segments_host runs behind the host polylines) as a stand-alone host program, meant to be
// built with -fsanitize=address,undefined: no GPU, no library, nothing loaded into another process.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I rebvio_amd/csrc
//       tests/cpp/edge_segments_host_check.cpp -o edge_segments_host_check && ./edge_segments_host_check
// Seeded random polylines - straight pieces with corners and noise, lines of one and two points, NaN and infinite positions, zero,
// negative and NaN sigmas, depths outside the clamp - in heap buffers of exactly the bytes that may be touched (np points, np spans,
// np nxt / line words, np keys, min(kept, cap) records: a read or write past any of them is caught). Checks the result's identities
// against the definition, that a second run gives the same bytes, that a cap cuts the records and not the counts, and that every
// outcome was reached. Prints "ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#include "edge_segments.hpp"

static int fails = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                \
    }                                                         \
  } while (0)

using namespace rh::esg;

static long seen_segments = 0, seen_split_rounds = 0, seen_unresolved = 0, seen_invalid = 0, seen_valid = 0, seen_dropped = 0, seen_capped = 0,
            seen_single = 0, seen_wild = 0;

template <class T>
static std::unique_ptr<T[]> exact(size_t n) {  // exactly n elements on the heap (one for n = 0: new T[0] may not be read at all)
  return std::unique_ptr<T[]>(new T[n + (n == 0)]);
}

static void run_map(std::mt19937& rng) {
  std::uniform_real_distribution<float> uni(0.0f, 1.0f);
  std::normal_distribution<float> noise(0.0f, 0.25f);
  const int nl = (int)(rng() % 6u);
  std::vector<SegPoint> pts;
  std::vector<rebvio_hip_polyline> lines_v;
  for (int l = 0; l < nl; ++l) {
    const int n = rng() % 5u == 0 ? 1 + (int)(rng() % 2u) : 1 + (int)(rng() % 90u);
    lines_v.push_back(rebvio_hip_polyline{(int)pts.size(), n, 0, 0});
    seen_single += n == 1;
    float x = 100.0f * (uni(rng) - 0.5f), y = 80.0f * (uni(rng) - 0.5f), dx = 2.0f * uni(rng) - 1.0f, dy = 2.0f * uni(rng) - 1.0f;
    const float r0 = 0.1f + 2.0f * uni(rng), r1 = 0.1f + 2.0f * uni(rng);
    for (int i = 0; i < n; ++i) {
      if (rng() % 20u == 0) { dx = 2.0f * uni(rng) - 1.0f; dy = 2.0f * uni(rng) - 1.0f; }
      x += dx; y += dy;
      SegPoint p{x + noise(rng), y + noise(rng), r0 + (r1 - r0) * (float)i / (float)n, 0.02f + 0.1f * uni(rng)};
      if (rng() % 60u == 0) {
        const float wild[] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), 1e30f};
        (rng() % 2u ? p.x : p.y) = wild[rng() % 4u];
        ++seen_wild;
      }
      if (rng() % 60u == 0) {
        const float wild[] = {0.0f, -0.05f, 1e-9f, std::numeric_limits<float>::quiet_NaN()};
        p.sigma = wild[rng() % 4u];
      }
      if (rng() % 80u == 0) p.rho = rng() % 2u ? 1e-4f : 50.0f;
      pts.push_back(p);
    }
  }
  const int np = (int)pts.size();
  const size_t N = (size_t)np;
  auto q = exact<SegPoint>(N);
  auto lines = exact<rebvio_hip_polyline>((size_t)nl);
  std::copy(pts.begin(), pts.end(), q.get());
  std::copy(lines_v.begin(), lines_v.end(), lines.get());
  rebvio_hip_segment_opts o;
  o.poly.filter = {2u, 0.5f, 1e-3f, 20.0f};
  o.poly.min_chain_length = 1;
  o.poly.reserved = 0;
  const float tols[] = {0.0f, 0.5f, 1.0f, 3.0f};
  o.tol = tols[rng() % 4u];
  o.min_length = rng() % 2u ? 4.0f : 0.0f;
  o.min_points = 2 + (int)(rng() % 8u);
  const int rounds[] = {1, 2, 4, 16, 32};
  o.max_rounds = rounds[rng() % 5u];
  const float R[9] = {0.36f, 0.48f, -0.8f, -0.8f, 0.6f, 0.0f, 0.48f, 0.64f, 0.6f}, t[3] = {0.5f, -1.25f, 2.0f};
  auto span = exact<SegSpan>(N);
  auto nxt = exact<int>(N), line_of = exact<int>(N);
  auto far = exact<unsigned long long>(N);
  auto segs = exact<rebvio_hip_line_segment>(N), segs2 = exact<rebvio_hip_line_segment>(N);
  rebvio_hip_segment_counts cnt, cnt2;
  segments_host(120.0f, q.get(), np, lines.get(), nl, o, R, t, 1.5f, span.get(), nxt.get(), line_of.get(), far.get(), segs.get(), np, &cnt);
  segments_host(120.0f, q.get(), np, lines.get(), nl, o, R, t, 1.5f, span.get(), nxt.get(), line_of.get(), far.get(), segs2.get(), np, &cnt2);
  CHECK(std::memcmp(&cnt, &cnt2, sizeof(cnt)) == 0 && (cnt.kept == 0 || std::memcmp(segs.get(), segs2.get(), (size_t)cnt.kept * sizeof(rebvio_hip_line_segment)) == 0));
  CHECK(cnt.points == np && cnt.lines == nl && cnt.kept <= cnt.segments_all && cnt.depth_valid <= cnt.kept && cnt.unresolved <= cnt.segments_all);
  CHECK(cnt.rounds_used >= 0 && cnt.rounds_used <= o.max_rounds && cnt.kept <= (np > 0 ? np - 1 : 0));
  // the final state: vertices partition every line; every interior point lies inside the segment of the vertex in front of it
  int all = 0;
  for (int l = 0; l < nl; ++l) {
    const int first = lines[l].first_point, last = first + lines[l].points - 1;
    CHECK(span[first].a == first && span[last].a == last);
    int v = first;
    for (int p = first; p <= last; ++p) {
      CHECK(line_of[p] == l);
      if (span[p].a == p) {
        CHECK(span[p].b == p && (p == first || nxt[v] == p));
        if (p != first) ++all;
        v = p;
      } else {
        CHECK(span[p].a == v && span[p].b == nxt[v] && v < p && p < nxt[v]);
      }
    }
    CHECK(nxt[last] == last);
  }
  CHECK(all == cnt.segments_all);
  const float tol2 = o.tol * o.tol;
  int valid = 0, prev_a = -1;
  for (int i = 0; i < cnt.kept; ++i) {
    const rebvio_hip_line_segment& s = segs[i];
    const int b = s.first_point + s.points - 1;
    CHECK(s.first_point > prev_a && span[s.first_point].a == s.first_point && nxt[s.first_point] == b && s.points >= o.min_points);
    prev_a = s.first_point;
    CHECK(s.line == line_of[s.first_point] && (s.flags & ~3) == 0 && s.chi2 >= 0.0f && s.max_dev2 >= 0.0f);
    CHECK(((s.flags & 2) != 0) == (s.max_dev2 > tol2));
    CHECK(std::memcmp(s.uv0, &q[s.first_point].x, 8) == 0 && std::memcmp(s.uv1, &q[b].x, 8) == 0);
    for (int p = s.first_point + 1; p < b; ++p) CHECK(!(seg_dev2(q[s.first_point], q[b], q[p]) > s.max_dev2));  // the maximum
    if (s.flags & 1) {
      ++valid;
      CHECK(s.rho0 >= 1e-3f && s.rho0 <= 20.0f && s.rho1 >= 1e-3f && s.rho1 <= 20.0f && s.sigma_rho0 >= 0.0f && s.sigma_rho1 >= 0.0f);
    } else {
      const float zeros[10] = {0};
      CHECK(std::memcmp(s.xyz0, zeros, 24) == 0 && std::memcmp(&s.rho0, zeros, 16) == 0);
    }
    seen_unresolved += (s.flags & 2) != 0;
  }
  CHECK(valid == cnt.depth_valid);
  seen_segments += cnt.segments_all;
  seen_split_rounds += cnt.rounds_used;
  seen_valid += valid;
  seen_invalid += cnt.kept - valid;
  seen_dropped += cnt.segments_all - cnt.kept;
  // a cap below the count: the same counts, the same leading records, nothing written behind the cap (an exact buffer)
  const int cap = cnt.kept / 2;
  auto segs_c = exact<rebvio_hip_line_segment>((size_t)cap);
  rebvio_hip_segment_counts cnt_c;
  segments_host(120.0f, q.get(), np, lines.get(), nl, o, R, t, 1.5f, span.get(), nxt.get(), line_of.get(), far.get(), segs_c.get(), cap, &cnt_c);
  CHECK(std::memcmp(&cnt, &cnt_c, sizeof(cnt)) == 0 && (cap == 0 || std::memcmp(segs.get(), segs_c.get(), (size_t)cap * sizeof(rebvio_hip_line_segment)) == 0));
  seen_capped += cap < cnt.kept;
}

int main() {
  std::mt19937 rng(24680);
  for (int rep = 0; rep < 1500; ++rep) run_map(rng);
  std::printf("segments %ld split rounds %ld unresolved %ld valid %ld invalid %ld dropped %ld capped %ld single %ld wild %ld\n", seen_segments,
              seen_split_rounds, seen_unresolved, seen_valid, seen_invalid, seen_dropped, seen_capped, seen_single, seen_wild);
  CHECK(seen_segments > 5000 && seen_split_rounds > 1000 && seen_unresolved > 50 && seen_valid > 1000 && seen_invalid > 50 && seen_dropped > 1000);
  CHECK(seen_capped > 500 && seen_single > 100 && seen_wild > 500);
  if (fails == 0) std::printf("ok\n");
  return fails ? 1 : 0;
}
