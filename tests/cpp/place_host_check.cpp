// The statements of place recognition (rebvio_amd/csrc/place.hpp: plc::counted, cell_of, bin_of, normalise, distance and the two host
// loops, which the kernels of track.hip and the hooks of api.hip compile) run as a stand-alone host program, meant to be built with
// -fsanitize=address,undefined: no GPU, no library, nothing loaded into another process.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I rebvio_amd/csrc
//       tests/cpp/place_host_check.cpp -o place_host_check && ./place_host_check
// Seeded random keyline tables of 0 .. 70000 keylines with NaN, infinite, denormal, zero, negative and huge values planted in pos,
// gradient and gradient_norm, in heap buffers of exactly the needed size, at image sizes from 1x1 to the accepted envelope's largest
// (4096 x 2548: the products yi * 6 and xi * 8 at their largest): every word index inside [0, 384), no float-to-int conversion of
// a value that does not fit, the words' sum within 384 of 65535. Databases of 0 .. 300 rows in heap buffers of exactly size * 768
// bytes: the records ascend strictly in (distance, index), stay inside the eligible rows and never pass min(k, eligible), which a
// result buffer of exactly that many records holds. Prints "ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>

#include "place.hpp"

static int fails = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                \
    }                                                         \
  } while (0)

int main() {
  using namespace rh;
  std::mt19937 rng(4711);
  std::uniform_real_distribution<float> uni(0.0f, 1.0f);
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float special[] = {nan, inf, -inf, 0.0f, -0.0f, std::numeric_limits<float>::denorm_min(), 1e-40f, -1e-40f,
                           std::numeric_limits<float>::max(), -std::numeric_limits<float>::max(), 3e9f, -3e9f, -1.0f, 2147483648.0f};
  const int n_special = (int)(sizeof(special) / sizeof(special[0]));
  const int sizes[][2] = {{1, 1}, {2, 3}, {32, 32}, {33, 37}, {48, 96}, {120, 160}, {480, 640}, {2548, 4096}};
  long counted_total = 0;
  for (const auto& sz : sizes) {
    const int rows = sz[0], cols = sz[1];
    // the corners of the image: the largest products the cell arithmetic forms
    CHECK(plc::cell_of(rows, cols, 0, 0) == 0 && (rows < 6 || cols < 8 || plc::cell_of(rows, cols, cols - 1, rows - 1) == 47));
    for (int n : {0, 1, 2, 63, 64, 65, 257, 1000, 70000}) {
      std::unique_ptr<rebvio_hip_keyline[]> kl(new rebvio_hip_keyline[(size_t)n + (n == 0)]);
      for (int i = 0; i < n; ++i) {
        rebvio_hip_keyline& q = kl[i];
        std::memset(&q, 0, sizeof(q));
        q.pos[0] = (cols + 4.0f) * uni(rng) - 2.0f;
        q.pos[1] = (rows + 4.0f) * uni(rng) - 2.0f;
        if (rng() % 4u == 0) q.pos[0] = std::floor(q.pos[0]), q.pos[1] = std::floor(q.pos[1]);
        if (rng() % 16u == 0) q.pos[0] = std::nextafter((float)cols, 0.0f), q.pos[1] = std::nextafter((float)rows, 0.0f);
        q.gradient[0] = 200.0f * uni(rng) - 100.0f;
        q.gradient[1] = rng() % 8u == 0 ? -q.gradient[0] : 200.0f * uni(rng) - 100.0f;
        q.gradient_norm = std::sqrt(q.gradient[0] * q.gradient[0] + q.gradient[1] * q.gradient[1]);
        if (rng() % 5u == 0) {
          const float v = special[rng() % (unsigned)n_special];
          switch (rng() % 5u) {
            case 0: q.pos[0] = v; break;
            case 1: q.pos[1] = v; break;
            case 2: q.gradient[0] = v; break;
            case 3: q.gradient[1] = v; break;
            default: q.gradient_norm = v; break;
          }
        }
        if (plc::counted(rows, cols, q.pos[0], q.pos[1], q.gradient[0], q.gradient[1], q.gradient_norm)) {
          const int w = plc::word_of(rows, cols, q.pos[0], q.pos[1], q.gradient[0], q.gradient[1]);
          CHECK(w >= 0 && w < plc::kWords);
          const int b = plc::bin_of(q.gradient[0], q.gradient[1]);
          CHECK(b >= 0 && b < 8 && (b >> 2) == (q.gradient[1] < 0.0f) && ((b >> 1) & 1) == (q.gradient[0] < 0.0f));
        }
      }
      std::unique_ptr<uint16_t[]> sig(new uint16_t[plc::kWords]);  // exactly 384 words on the heap
      int counted = -1;
      plc::signature_host(rows, cols, kl.get(), n, sig.get(), &counted);
      CHECK(counted >= 0 && counted <= n);
      long sum = 0;
      for (int k = 0; k < plc::kWords; ++k) sum += sig[k];
      CHECK(counted == 0 ? sum == 0 : (sum > 65535 - plc::kWords && sum <= 65535));
      counted_total += counted;
    }
  }
  CHECK(counted_total > 100000);
  // normalise at its corners: h <= n <= 65536 (keylines_max's ceiling) and beyond
  CHECK(plc::normalise(0, 0) == 0 && plc::normalise(1, 1) == 65535 && plc::normalise(65536, 65536) == 65535);
  CHECK(plc::normalise(1, 3) == 21845 && plc::normalise(1, 65536) == 0 && plc::normalise(0xFFFFFFFFu, 0xFFFFFFFFu) == 65535);

  // the query
  long records = 0;
  for (int size : {0, 1, 3, 4, 5, 63, 64, 65, 257, 300}) {
    std::unique_ptr<uint16_t[]> tab(new uint16_t[(size_t)size * plc::kWords + (size == 0)]);
    std::unique_ptr<uint16_t[]> q(new uint16_t[plc::kWords]);
    for (int k = 0; k < plc::kWords; ++k) q[k] = (uint16_t)(rng() & 0xffffu);
    for (size_t k = 0; k < (size_t)size * plc::kWords; ++k) tab[k] = (uint16_t)(rng() & 0xffffu);
    if (size >= 5) {  // a copy of the query, a copy of another row (a tie), the two extreme rows
      std::memcpy(&tab[(size_t)2 * plc::kWords], q.get(), plc::kWords * sizeof(uint16_t));
      std::memcpy(&tab[(size_t)4 * plc::kWords], &tab[(size_t)1 * plc::kWords], plc::kWords * sizeof(uint16_t));
      for (int k = 0; k < plc::kWords; ++k) tab[k] = 65535, tab[(size_t)3 * plc::kWords + k] = 0;
    }
    for (int k : {1, 2, 16}) {
      for (int ex : {0, 1, size, size + 3}) {
        const int eligible = size - ex > 0 ? size - ex : 0;
        const int want = k < eligible ? k : eligible;
        // exactly min(k, eligible) records on the heap: one written past them is caught
        std::unique_ptr<rebvio_hip_place_match[]> out(new rebvio_hip_place_match[(size_t)want + (want == 0)]);
        int count = -1;
        plc::query_host(tab.get(), size, q.get(), k, ex, out.get(), &count);
        CHECK(count == want);
        for (int r = 0; r < count; ++r) {
          CHECK(out[r].index >= 0 && out[r].index < eligible && out[r].tag == 0);
          CHECK(out[r].distance == plc::distance(&tab[(size_t)out[r].index * plc::kWords], q.get()));
          CHECK(out[r].distance <= 384u * 65535u);
          if (r > 0)
            CHECK(out[r - 1].distance < out[r].distance || (out[r - 1].distance == out[r].distance && out[r - 1].index < out[r].index));
        }
        if (size >= 5 && ex == 0) CHECK(out[0].index == 2 && out[0].distance == 0);
        records += count;
      }
    }
  }
  // the largest distance there is
  {
    std::unique_ptr<uint16_t[]> a(new uint16_t[plc::kWords]), b(new uint16_t[plc::kWords]);
    for (int k = 0; k < plc::kWords; ++k) a[k] = 65535, b[k] = 0;
    CHECK(plc::distance(a.get(), b.get()) == 384u * 65535u && plc::distance(b.get(), a.get()) == 384u * 65535u);
    CHECK(plc::distance(a.get(), a.get()) == 0);
  }
  CHECK(records > 100);
  if (fails == 0) std::printf("%ld keylines counted, %ld records\nok\n", counted_total, records);
  return fails ? 1 : 0;
}
