// The host side of rebvio_hip_map_edge_chains / rebvio_hip_map_edge_polylines (rebvio_amd/csrc/edge_chains.hpp: the per-keyline
// statements and ech::chains_host / ech::polylines_host over them - what rebvio_hip_test_edge_chains_host / _edge_polylines_host run)
// as a stand-alone host program, meant to be built with -fsanitize=address,undefined: no GPU, no library, nothing loaded into
// another process.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I rebvio_amd/csrc
//       tests/cpp/edge_chains_host_check.cpp -o edge_chains_host_check && ./edge_chains_host_check
// Seeded random link tables with arbitrary integers in both fields (INT_MIN, INT_MAX, -1, n, indices just outside), and adversarial
// ones - one path in shuffled order, one cycle over everything, 2- and 3-cycles beside paths, every keyline naming one target, self
// links - all in heap buffers of exactly the needed size (a read or write past a link array, a state buffer or the table is caught).
// Checks the table's identities against a plain walk of succ, that a second run gives the same bytes, the polylines' bookkeeping,
// and that every outcome was reached. Prints "ok".
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <numeric>
#include <random>
#include <vector>

#include "edge_chains.hpp"

static int fails = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                \
    }                                                         \
  } while (0)

using rh::ech::ChainNode;

static long seen_paths = 0, seen_cycles = 0, seen_singletons = 0, seen_long = 0, seen_unanswered = 0, seen_wild = 0, seen_lines = 0,
            seen_closed = 0, seen_split = 0, seen_short = 0, seen_capped = 0;

template <class T>
static std::unique_ptr<T[]> exact(size_t n) {  // exactly n elements on the heap (one for n = 0: new T[0] may not be read at all)
  return std::unique_ptr<T[]>(new T[n + (n == 0)]);
}

static void run_table(const std::vector<int>& idp_v, const std::vector<int>& idn_v, std::mt19937& rng) {
  const int n = (int)idp_v.size();
  const size_t N = (size_t)n;
  auto idp = exact<int>(N), idn = exact<int>(N);
  std::copy(idp_v.begin(), idp_v.end(), idp.get());
  std::copy(idn_v.begin(), idn_v.end(), idn.get());
  auto a = exact<ChainNode>(N), b = exact<ChainNode>(N);
  auto succ = exact<int>(N), len = exact<int>(N), start_of = exact<int>(N), order = exact<int>(N), order2 = exact<int>(N);
  auto starts = exact<int>(N + 1), starts2 = exact<int>(N + 1);
  auto refs = exact<rebvio_hip_chain_ref>(N), refs2 = exact<rebvio_hip_chain_ref>(N);
  int nc = -1, nc2 = -1;
  rh::ech::chains_host(idp.get(), idn.get(), n, a.get(), b.get(), succ.get(), len.get(), start_of.get(), refs.get(), order.get(), starts.get(), &nc);
  rh::ech::chains_host(idp.get(), idn.get(), n, a.get(), b.get(), succ.get(), len.get(), start_of.get(), refs2.get(), order2.get(), starts2.get(), &nc2);
  CHECK(nc == nc2 && (N == 0 || std::memcmp(refs.get(), refs2.get(), N * sizeof(rebvio_hip_chain_ref)) == 0));
  CHECK(N == 0 || std::memcmp(order.get(), order2.get(), N * sizeof(int)) == 0);
  CHECK(std::memcmp(starts.get(), starts2.get(), ((size_t)nc + 1) * sizeof(int)) == 0);
  // the definition, walked: succ from the fields, the table's identities
  CHECK(nc >= 0 && nc <= n && starts[nc] == n && (nc == 0 || starts[0] == 0));
  std::vector<char> hit(N, 0);
  for (int i = 0; i < n; ++i) {
    const long long s = idn[i];
    const bool linked = s >= 0 && s < n && s != i && idp[s] == i;
    CHECK(succ[i] == (linked ? (int)s : -1));
    if (s >= 0 && s < n && !linked) ++seen_unanswered;
    if (s < -1 || s > n) ++seen_wild;
    CHECK(order[i] >= 0 && order[i] < n && !hit[(size_t)order[i]]);
    if (order[i] >= 0 && order[i] < n) hit[(size_t)order[i]] = 1;
  }
  int prev_head = -1;
  for (int c = 0; c < nc; ++c) {
    const int s0 = starts[c], L = starts[c + 1] - s0;
    CHECK(L >= 1 && s0 >= 0 && s0 + L <= n);
    if (!(L >= 1 && s0 >= 0 && s0 + L <= n)) return;
    const int head = order[s0];
    CHECK(head > prev_head);
    prev_head = head;
    const int cyc = refs[head].flags & 1;
    int smallest = head;
    for (int r = 0; r < L; ++r) {
      const int k = order[s0 + r];
      CHECK(refs[k].head == head && refs[k].rank == r && refs[k].length == L && refs[k].flags == cyc);
      CHECK(succ[k] == (r + 1 < L ? order[s0 + r + 1] : (cyc ? head : -1)));
      smallest = std::min(smallest, k);
    }
    CHECK(!cyc || smallest == head);
    if (cyc) ++seen_cycles; else if (L == 1) ++seen_singletons; else ++seen_paths;
    if (L > 64) ++seen_long;
  }
  // polylines over the same table: random depths, a filter that drops some, a min length that drops some chains, caps that cut
  std::uniform_real_distribution<float> uni(0.0f, 1.0f);
  auto pos_img = exact<float>(2 * N), rs = exact<float>(2 * N), gn = exact<float>(N);
  auto mt = exact<unsigned>(N);
  for (int i = 0; i < n; ++i) {
    pos_img[2 * i] = 100.0f * (uni(rng) - 0.5f);
    pos_img[2 * i + 1] = 80.0f * (uni(rng) - 0.5f);
    rs[2 * i] = 0.05f + 3.0f * uni(rng);
    rs[2 * i + 1] = rs[2 * i] * 0.7f * uni(rng);
    gn[i] = 9.0f * uni(rng);
    mt[i] = rng() % 6u;
    if (rng() % 40u == 0) rs[2 * i + (int)(rng() % 2u)] = std::numeric_limits<float>::quiet_NaN();
  }
  rebvio_hip_polyline_opts o;
  o.filter = {rng() % 3u == 0 ? 0u : 2u, rng() % 3u == 0 ? 1e9f : 0.5f, 1e-3f, 20.0f};
  o.min_chain_length = 1 + (int)(rng() % 9u);
  o.reserved = 0;
  const float R[9] = {0.36f, 0.48f, -0.8f, -0.8f, 0.6f, 0.0f, 0.48f, 0.64f, 0.6f}, t[3] = {0.5f, -1.25f, 2.0f};
  int np_all = -1, nl_all = -1;
  auto pts = exact<rebvio_hip_cloud_point>(N);
  auto r2 = exact<int>(2 * N);
  auto lines = exact<rebvio_hip_polyline>(N);
  rh::ech::polylines_host(120.0f, pos_img.get(), rs.get(), gn.get(), mt.get(), n, refs.get(), order.get(), o, R, t, 1.5f, pts.get(), r2.get(), n,
                          lines.get(), n, &np_all, &nl_all);
  CHECK(np_all >= 0 && np_all <= n && nl_all >= 0 && nl_all <= np_all);
  int at = 0;
  for (int l = 0; l < nl_all; ++l) {
    const rebvio_hip_polyline& ln = lines[l];
    CHECK(ln.first_point == at && ln.points >= 1 && (ln.flags & ~1) == 0);
    const rebvio_hip_chain_ref hr = refs[ln.head];
    CHECK(hr.head == ln.head && hr.length >= o.min_chain_length);
    for (int k = 0; k < ln.points && at + k < np_all; ++k) {
      const rebvio_hip_cloud_point& p = pts[at + k];
      CHECK(r2[2 * (at + k)] == ln.head && refs[p.keyline].head == ln.head && refs[p.keyline].rank == r2[2 * (at + k) + 1]);
      CHECK(k == 0 || r2[2 * (at + k) + 1] == r2[2 * (at + k - 1) + 1] + 1);  // consecutive ranks
      CHECK(rh::kfp::filter_pass(o.filter, p.rho, p.sigma_rho, p.matches) && p.rho == rs[2 * p.keyline]);
    }
    if (ln.flags & 1) {
      CHECK((hr.flags & 1) && ln.points == hr.length);
      ++seen_closed;
    }
    if (ln.points < hr.length) ++seen_split;
    at += ln.points;
    ++seen_lines;
  }
  CHECK(at == np_all);
  for (int c = 0; c < nc; ++c) seen_short += starts[c + 1] - starts[c] < o.min_chain_length;
  // caps below the counts: the same counts, the same leading records, nothing written behind the caps (exact buffers)
  const int cp = np_all / 2, cl = nl_all / 2;
  auto pts_c = exact<rebvio_hip_cloud_point>((size_t)cp);
  auto r2_c = exact<int>(2 * (size_t)cp);
  auto lines_c = exact<rebvio_hip_polyline>((size_t)cl);
  int np_c = -1, nl_c = -1;
  rh::ech::polylines_host(120.0f, pos_img.get(), rs.get(), gn.get(), mt.get(), n, refs.get(), order.get(), o, R, t, 1.5f, pts_c.get(), r2_c.get(), cp,
                          lines_c.get(), cl, &np_c, &nl_c);
  CHECK(np_c == np_all && nl_c == nl_all);
  CHECK(cp == 0 || std::memcmp(pts_c.get(), pts.get(), (size_t)cp * sizeof(rebvio_hip_cloud_point)) == 0);
  CHECK(cl == 0 || std::memcmp(lines_c.get(), lines.get(), (size_t)cl * sizeof(rebvio_hip_polyline)) == 0);
  seen_capped += cp < np_all;
}

int main() {
  std::mt19937 rng(97531);
  const int wild[] = {INT_MIN, INT_MAX, -1, -2, INT_MIN + 1, INT_MAX - 1};
  for (int rep = 0; rep < 400; ++rep) {  // random tables
    const int n = rep < 8 ? rep : (int)(rng() % 400u);
    std::vector<int> idp((size_t)n), idn((size_t)n);
    for (int i = 0; i < n; ++i) {
      idp[i] = (int)(rng() % (unsigned)(n + 4)) - 2;
      idn[i] = (int)(rng() % (unsigned)(n + 4)) - 2;
      if (rng() % 10u == 0) idp[i] = wild[rng() % 6u];
      if (rng() % 10u == 0) idn[i] = wild[rng() % 6u];
      if (rng() % 50u == 0) idn[i] = idp[i] = i;
    }
    for (int i = 0; i < n; ++i)  // answer most links so that chains form
      if (rng() % 10u < 7 && idn[i] >= 0 && idn[i] < n) idp[idn[i]] = i;
    run_table(idp, idn, rng);
  }
  for (int n : {1, 2, 3, 64, 255, 256, 257, 1000, 1024, 5000}) {  // adversarial tables
    std::vector<int> perm((size_t)n);
    std::iota(perm.begin(), perm.end(), 0);
    std::shuffle(perm.begin(), perm.end(), rng);
    auto table = [&](bool cycle, bool descending) {
      std::vector<int> idp((size_t)n, -1), idn((size_t)n, -1);
      for (int r = 0; r + 1 < n + (cycle ? 1 : 0); ++r) {
        const int x = descending ? n - 1 - r % n : perm[(size_t)(r % n)], y = descending ? n - 1 - (r + 1) % n : perm[(size_t)((r + 1) % n)];
        if (x == y) continue;
        idn[x] = y;
        idp[y] = x;
      }
      run_table(idp, idn, rng);
    };
    table(false, false);  // one path in shuffled order: every round moves something
    table(true, false);   // one cycle over everything
    table(false, true);   // a path in descending index order
    std::vector<int> idp((size_t)n, -1), idn((size_t)n, 0);  // every keyline names keyline 0; id_prev[0] keeps the last
    idp[0] = n - 1;
    run_table(idp, idn, rng);
    std::vector<int> p3((size_t)n, -1), n3((size_t)n, -1);  // 2- and 3-cycles beside paths
    for (int i = 0; i + 5 <= n; i += 9) {
      n3[i] = i + 1; p3[i + 1] = i; n3[i + 1] = i; p3[i] = i + 1;
      n3[i + 2] = i + 4; p3[i + 4] = i + 2; n3[i + 4] = i + 3; p3[i + 3] = i + 4; n3[i + 3] = i + 2; p3[i + 2] = i + 3;
      for (int k = i + 5; k + 1 < std::min(n, i + 9); ++k) {
        n3[k] = k + 1;
        p3[k + 1] = k;
      }
    }
    run_table(p3, n3, rng);
  }
  std::printf("paths %ld cycles %ld singletons %ld long %ld unanswered %ld wild %ld lines %ld closed %ld split %ld short %ld capped %ld\n",
              seen_paths, seen_cycles, seen_singletons, seen_long, seen_unanswered, seen_wild, seen_lines, seen_closed, seen_split, seen_short,
              seen_capped);
  CHECK(seen_paths > 1000 && seen_cycles > 100 && seen_singletons > 1000 && seen_long > 10 && seen_unanswered > 1000 && seen_wild > 1000);
  CHECK(seen_lines > 1000 && seen_closed > 10 && seen_split > 100 && seen_short > 100 && seen_capped > 100);
  if (fails == 0) std::printf("ok\n");
  return fails ? 1 : 0;
}
