// The host side of rebvio_hip_map_keyframe_align_many (rebvio_amd/csrc/kf_many.hpp: the ranking, the 13 starts and one hypothesis of
// the host hook - the functions rebvio_hip_kf_align_best, rebvio_hip_kf_hypotheses_around and rebvio_hip_test_kf_align_many_host
// compile) run as a stand-alone host program, meant to be built with -fsanitize=address,undefined: no GPU, no library, nothing
// loaded into another process.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I rebvio_amd/csrc
//       tests/cpp/kf_many_host_check.cpp -o kf_many_host_check && ./kf_many_host_check
// Seeded random distance fields (ids with empty cells, distances) over random keylines, and snapshots of 0 .. 600 keyframe keylines
// with NaN, infinite, huge and out-of-frame values planted in every field, all in heap buffers of exactly the needed size (a read
// past a snapshot, a keyline array or the field is caught); guesses near the identity and far from it. Checks that inliers never
// exceeds used nor used the size, that a second run gives the same bytes, that the ranking is the brute-force one on random result
// arrays (ties, statuses, NaN costs) and that the 13 starts are what the definition says. Prints "ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#include "kf_many.hpp"

static int fails = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                \
    }                                                         \
  } while (0)

int main() {
  std::mt19937 rng(4321);
  std::uniform_real_distribution<float> uni(0.0f, 1.0f);
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float special[] = {nan, inf, -inf, 0.0f, -0.0f, std::numeric_limits<float>::denorm_min(), std::numeric_limits<float>::max(),
                           -std::numeric_limits<float>::max(), 1e30f, -1e30f, 1e6f, -1e6f};
  const int n_special = (int)(sizeof(special) / sizeof(special[0]));
  long terms = 0, inliers_seen = 0;
  for (int field = 0; field < 60; ++field) {
    const int rows = 8 + (int)(rng() % 40u), cols = 8 + (int)(rng() % 50u), n_cur = 1 + (int)(rng() % 300u);
    const size_t cells = (size_t)rows * (size_t)cols;
    std::unique_ptr<int[]> ids(new int[cells]), dists(new int[cells]);
    std::unique_ptr<rh::kfp::AlignF2[]> pos(new rh::kfp::AlignF2[(size_t)n_cur]), unit(new rh::kfp::AlignF2[(size_t)n_cur]);
    for (size_t c = 0; c < cells; ++c) {
      ids[c] = rng() % 5u == 0 ? -1 : (int)(rng() % (unsigned)n_cur);
      dists[c] = (int)(rng() % 12u);
    }
    for (int i = 0; i < n_cur; ++i) {
      const float a = 6.2831853f * uni(rng);
      pos[i] = {cols * uni(rng), rows * uni(rng)};
      unit[i] = {std::cos(a), std::sin(a)};
      if (field % 3 == 1 && rng() % 7u == 0) unit[i] = {0.0f, 0.0f};
      if (field % 3 == 2 && rng() % 7u == 0) (rng() % 2u ? pos[i].x : unit[i].y) = special[rng() % (unsigned)n_special];
    }
    rh::kfp::AlignMap am;
    am.fm = 0.9f * cols; am.cx = cols / 2.0f; am.cy = rows / 2.0f; am.rows = rows; am.cols = cols;
    am.df = nullptr; am.df_nr = 1; am.ids = ids.get(); am.dists = dists.get();
    am.pos = pos.get(); am.unit = unit.get(); am.cap = n_cur;
    for (int n : {0, 1, 11, 64, 257, 600}) {
      // exactly n keyframe keylines on the heap
      std::unique_ptr<float[]> prs4(new float[4 * (size_t)n + (n == 0)]), nrm(new float[2 * (size_t)n + (n == 0)]);
      std::unique_ptr<unsigned[]> mt(new unsigned[(size_t)n + (n == 0)]);
      for (int j = 0; j < n; ++j) {
        prs4[4 * j] = 1.4f * cols * (uni(rng) - 0.5f);  // some project out of the frame
        prs4[4 * j + 1] = 1.4f * rows * (uni(rng) - 0.5f);
        prs4[4 * j + 2] = std::exp(-3.0f + 4.0f * uni(rng));
        prs4[4 * j + 3] = 0.3f * prs4[4 * j + 2] * uni(rng);
        mt[j] = rng() % 6u;
        const float a = 6.2831853f * uni(rng);
        nrm[2 * j] = std::cos(a);
        nrm[2 * j + 1] = std::sin(a);
        if (field % 2 == 1 && rng() % 4u == 0) prs4[4 * j + (int)(rng() % 4u)] = special[rng() % (unsigned)n_special];
        if (field % 2 == 1 && rng() % 9u == 0) nrm[2 * j + (int)(rng() % 2u)] = special[rng() % (unsigned)n_special];
      }
      rebvio_hip_kf_align_opts o;
      std::memset(&o, 0, sizeof(o));
      o.kf_filter = {field % 4 == 0 ? 0u : 2u, 0.5f, 1e-3f, 20.0f};
      o.huber_px = field % 5 == 0 ? 0.3 : 2.0;
      o.min_cos = field % 6 == 0 ? -1.0 : 0.5;
      o.max_dist = 11 - field % 4;
      o.max_iter = field % 3 == 0 ? 0 : 8;
      o.min_used = field % 7 == 0 ? 0 : 12;
      rebvio_hip_kf_hypothesis h13[13];
      const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0.01 * (field % 3), -0.02, 0.03 * (field % 2)};
      rh::kfm::around(nullptr, I, t, field % 2 ? 0.03 : 1.5, field % 2 ? 0.12 : 40.0, h13);
      std::vector<rebvio_hip_kf_hyp_result> res(13), again(13);
      for (int h = 0; h < 13; ++h) {
        rh::kfm::align_host(am, prs4.get(), mt.get(), field % 4 == 3 ? nullptr : nrm.get(), n, o, h13[h].R0, h13[h].t0, &res[(size_t)h].pose, nullptr,
                             &res[(size_t)h].inliers);
        rh::kfm::align_host(am, prs4.get(), mt.get(), field % 4 == 3 ? nullptr : nrm.get(), n, o, h13[h].R0, h13[h].t0, &again[(size_t)h].pose, nullptr,
                             &again[(size_t)h].inliers);
        const rebvio_hip_kf_hyp_result& r = res[(size_t)h];
        CHECK(std::memcmp(&r, &again[(size_t)h], sizeof(r)) == 0);
        CHECK(r.pose.candidates == n && r.pose.used >= 0 && r.pose.used <= n && r.inliers >= 0 && r.inliers <= r.pose.used && r.reserved == 0);
        CHECK(r.pose.status == 0 || r.pose.status == 2 || r.pose.status == 3);
        CHECK(n > 0 || (r.pose.status == 3 && r.pose.used == 0 && r.inliers == 0 && r.pose.cost == 0.0));
        CHECK(r.pose.iterations >= 0 && r.pose.iterations <= o.max_iter);
        terms += r.pose.used;
        inliers_seen += r.inliers;
      }
      const int b = rh::kfm::best(res.data(), 13, 12);
      CHECK(b >= -1 && b < 13);
      if (b >= 0) CHECK(res[(size_t)b].pose.status == 0 && res[(size_t)b].inliers >= 12);
    }
  }
  CHECK(terms > 10000 && inliers_seen > 100 && inliers_seen < terms);

  // the ranking against brute force, on result arrays in buffers of exactly n results
  for (int round = 0; round < 2000; ++round) {
    const int n = 1 + (int)(rng() % 64u), min_inliers = (int)(rng() % 6u);
    std::unique_ptr<rebvio_hip_kf_hyp_result[]> res(new rebvio_hip_kf_hyp_result[(size_t)n]);
    std::memset(res.get(), 0, (size_t)n * sizeof(rebvio_hip_kf_hyp_result));
    for (int h = 0; h < n; ++h) {
      res[h].pose.status = rng() % 3u == 0 ? (rng() % 2u ? 2 : 3) : 0;
      res[h].inliers = (int)(rng() % 8u);
      res[h].pose.cost = rng() % 11u == 0 ? (double)nan : (double)(rng() % 4u);
    }
    bool any_nan = false;  // a NaN cost never wins a comparison: only the properties below are asked then
    for (int k = 0; k < n; ++k) any_nan = any_nan || (res[k].pose.status == 0 && std::isnan(res[k].pose.cost));
    int want = any_nan ? -2 : -1;
    for (int h = 0; h < n && want == -1; ++h) {
      if (res[h].pose.status != 0 || res[h].inliers < min_inliers) continue;
      bool beaten = false;  // by a qualifying result that ranks strictly ahead, or equally and earlier
      for (int k = 0; k < n && !beaten; ++k) {
        if (k == h || res[k].pose.status != 0 || res[k].inliers < min_inliers) continue;
        beaten = res[k].inliers > res[h].inliers ||
                 (res[k].inliers == res[h].inliers &&
                  (res[k].pose.cost < res[h].pose.cost || (res[k].pose.cost == res[h].pose.cost && k < h)));
      }
      if (!beaten) want = h;
    }
    const int got = rh::kfm::best(res.get(), n, min_inliers);
    if (want != -2) CHECK(got == want);
    if (got >= 0) {
      CHECK(res[got].pose.status == 0 && res[got].inliers >= min_inliers);
      for (int k = 0; k < n; ++k) CHECK(res[k].pose.status != 0 || res[k].inliers <= res[got].inliers);
    }
  }

  // the 13 starts
  {
    const double R[9] = {0.36, 0.48, -0.8, -0.8, 0.6, 0.0, 0.48, 0.64, 0.6}, t[3] = {0.5, -1.0, 2.0};
    rebvio_hip_kf_hypothesis out[13];
    rh::kfm::around(nullptr, R, t, 0.03, 0.12, out);
    CHECK(std::memcmp(out[0].R0, R, sizeof(R)) == 0 && std::memcmp(out[0].t0, t, sizeof(t)) == 0 && out[0].snap == nullptr);
    for (int k = 0; k < 13; ++k) {
      double worst = 0;
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
          double s = 0;
          for (int l = 0; l < 3; ++l) s += out[k].R0[3 * i + l] * out[k].R0[3 * j + l];
          worst = std::fmax(worst, std::fabs(s - (i == j ? 1.0 : 0.0)));
        }
      CHECK(worst < 1e-15);
      if (k < 7) CHECK(std::memcmp(out[k].t0, t, sizeof(t)) == 0);
      if (k >= 7) CHECK(std::memcmp(out[k].R0, R, sizeof(R)) == 0 && out[k].t0[(k - 7) / 2] == t[(k - 7) / 2] + ((k - 7) % 2 ? -0.12 : 0.12));
    }
    rh::kfm::around(nullptr, R, t, 0.0, 0.0, out);
    for (int k = 1; k < 13; ++k) CHECK(std::memcmp(&out[k], &out[0], sizeof(out[0])) == 0);
  }
  if (fails == 0) std::printf("ok (%ld terms, %ld inliers)\n", terms, inliers_seen);
  return fails ? 1 : 0;
}
