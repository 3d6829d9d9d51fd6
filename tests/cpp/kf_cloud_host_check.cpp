// The per-record statement of a snapshot's point cloud (rebvio_amd/csrc/kf_cloud.hpp: kfc::record, the function k_kf_cloud_emit and
// rebvio_hip_test_kf_cloud_host compile) run as a stand-alone host program, meant to be built with -fsanitize=address,undefined:
// no GPU, no library, nothing loaded into another process.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I rebvio_amd/csrc
//       tests/cpp/kf_cloud_host_check.cpp -o kf_cloud_host_check && ./kf_cloud_host_check
// Seeded random snapshots of 0 .. 1000 keylines with NaN, infinite, denormal, zero, negative and huge values planted in every field,
// in heap buffers of exactly the needed size (so a write past min(count, cap) records or a read past n keylines is caught), at
// caps of 0, 1, the count itself and above the count. Checks that count does not depend on cap, that the records of a smaller cap are
// a prefix of the full cloud, that keyline increases strictly and that every point passes the filter. Prints "ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#include "kf_cloud.hpp"

static int fails = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                \
    }                                                         \
  } while (0)

int main() {
  std::mt19937 rng(12345);
  std::uniform_real_distribution<float> uni(0.0f, 1.0f);
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float special[] = {nan, inf, -inf, 0.0f, -0.0f, std::numeric_limits<float>::denorm_min(), 1e-40f, -1e-40f,
                           std::numeric_limits<float>::max(), -std::numeric_limits<float>::max(), 1e30f, -1.0f, 1e-3f, 20.0f};
  const int n_special = (int)(sizeof(special) / sizeof(special[0]));
  const rebvio_hip_cloud_filter filters[] = {{2u, 0.5f, 1e-3f, 20.0f}, {0u, inf, 1e-30f, inf}, {3u, 0.0f, 0.1f, 4.0f}, {0xFFFFFFFFu, 1.0f, 1.0f, 1.0f}};
  long points = 0;
  for (int n : {0, 1, 2, 63, 64, 65, 255, 256, 257, 1000}) {
    for (int round = 0; round < 4; ++round) {
      // exactly n keylines on the heap: nothing to read behind them
      std::unique_ptr<float[]> prs4(new float[4 * (size_t)n + (n == 0)]);
      std::unique_ptr<unsigned[]> mt(new unsigned[(size_t)n + (n == 0)]);
      for (int j = 0; j < n; ++j) {
        prs4[4 * j] = 200.0f * uni(rng) - 100.0f;
        prs4[4 * j + 1] = 200.0f * uni(rng) - 100.0f;
        prs4[4 * j + 2] = std::exp(-7.0f + 11.0f * uni(rng));
        prs4[4 * j + 3] = prs4[4 * j + 2] * uni(rng);
        mt[j] = rng() % 6u;
        if (round > 0 && rng() % 3u == 0) prs4[4 * j + (int)(rng() % 4u)] = special[rng() % (unsigned)n_special];
        if (round > 1 && rng() % 5u == 0) mt[j] = 0xFFFFFFFFu;
      }
      const rebvio_hip_cloud_filter& f = filters[round];
      float R[9], t[3];
      for (float& v : R) v = 2.0f * uni(rng) - 1.0f;
      for (float& v : t) v = 10.0f * uni(rng) - 5.0f;
      if (round == 3) R[4] = inf, t[1] = std::numeric_limits<float>::max();  // (the entries refuse a NaN pose only)
      const float fm = round == 2 ? 1e-30f : 137.5f, scale = round == 1 ? 1e30f : 0.37f;
      int count = -1;
      rh::kfc::extract_host(fm, prs4.get(), mt.get(), n, f, R, t, scale, nullptr, 0, &count);
      CHECK(count >= 0 && count <= n);
      std::vector<rebvio_hip_cloud_point> full((size_t)count);
      int c2 = -1;
      rh::kfc::extract_host(fm, prs4.get(), mt.get(), n, f, R, t, scale, full.data(), count, &c2);
      CHECK(c2 == count);
      int last = -1;
      for (const rebvio_hip_cloud_point& p : full) {
        CHECK(p.keyline > last && p.keyline < n);
        last = p.keyline;
        CHECK(rh::kfp::filter_pass(f, p.rho, p.sigma_rho, p.matches) && p.rho > 0.0f && !std::isnan(p.sigma_rho));
        CHECK(std::memcmp(&p.rho, &prs4[4 * p.keyline + 2], 4) == 0 && std::memcmp(&p.sigma_rho, &prs4[4 * p.keyline + 3], 4) == 0);
        CHECK(p.matches == mt[p.keyline] && p.gradient_norm == 0.0f && !std::signbit(p.gradient_norm));
      }
      points += count;
      for (int cap : {0, 1, count / 2, count + 7}) {
        // exactly cap records on the heap: a record written past them is caught
        std::unique_ptr<rebvio_hip_cloud_point[]> out(new rebvio_hip_cloud_point[(size_t)cap + (cap == 0)]);
        int c3 = -1;
        rh::kfc::extract_host(fm, prs4.get(), mt.get(), n, f, R, t, scale, cap ? out.get() : nullptr, cap, &c3);
        CHECK(c3 == count);
        const int k = count < cap ? count : cap;
        CHECK(k == 0 || std::memcmp(out.get(), full.data(), (size_t)k * sizeof(rebvio_hip_cloud_point)) == 0);
      }
    }
  }
  CHECK(points > 1000);
  if (fails == 0) std::printf("ok (%ld points)\n", points);
  return fails ? 1 : 0;
}
