// Place recognition (rebvio_hip_map_place_signature, rebvio_hip_place_db_*; include/rebvio_hip.h is the definition): the statements
// of a map's edge signature - which keylines count, their image cell and orientation bin, the normalisation of the histogram -
// and of the L1 distance between two signatures. One source for the device (k_place_hist / k_place_norm / k_place_dist /
// k_place_topk, track.hip) and the host (rebvio_hip_test_place_signature_host / _query_host, api.hip; the stand-alone sanitizer
// program of tests/cpp), as kf_cloud.hpp and stereo_prior.hpp do it. Integer arithmetic behind the comparisons: no output word
// depends on the order in which keylines or rows are visited.
#pragma once

#include <math.h>
#include <stdint.h>

#include "hostmath.hpp"  // RH_HD
#include "rebvio_hip.h"

namespace rh {
namespace plc {

constexpr int kCellsX = 8, kCellsY = 6, kBins = 8;
constexpr int kWords = kCellsX * kCellsY * kBins;
static_assert(kWords == REBVIO_HIP_PLACE_WORDS, "8 x 6 cells x 8 orientation bins");

// Whether a keyline enters the histogram. Every test is positive: a NaN anywhere fails it.
RH_HD inline bool counted(int rows, int cols, float px, float py, float gx, float gy, float gnorm) {
  const float inf = __builtin_huge_valf();
  if (!(px >= 0.0f && px < (float)cols && py >= 0.0f && py < (float)rows)) return false;
  if (!(gnorm > 0.0f)) return false;
  if (!(fabsf(gx) < inf && fabsf(gy) < inf)) return false;
  return fabsf(gx) > 0.0f || fabsf(gy) > 0.0f;
}

// The image cell of pixel (xi, yi), 0 <= xi < cols, 0 <= yi < rows: 8 columns x 6 rows of cells, row-major.
RH_HD inline int cell_of(int rows, int cols, int xi, int yi) { return ((yi * kCellsY) / rows) * kCellsX + (xi * kCellsX) / cols; }

// The orientation octant of a gradient from comparisons alone: the two signs (-0.0 is not negative), then which component is
// the larger (a tie: 0).
RH_HD inline int bin_of(float gx, float gy) { return 4 * (gy < 0.0f ? 1 : 0) + 2 * (gx < 0.0f ? 1 : 0) + (fabsf(gy) > fabsf(gx) ? 1 : 0); }

// The histogram word of a counted keyline.
RH_HD inline int word_of(int rows, int cols, float px, float py, float gx, float gy) {
  return cell_of(rows, cols, (int)px, (int)py) * kBins + bin_of(gx, gy);
}

// One signature word from its histogram count h and the number n of counted keylines (h <= n).
RH_HD inline uint16_t normalise(uint32_t h, uint32_t n) { return n ? (uint16_t)(((uint64_t)h * 65535u) / n) : (uint16_t)0; }

// sum |a[k] - b[k]| over the 384 words
RH_HD inline uint32_t distance(const uint16_t* a, const uint16_t* b) {
  uint32_t d = 0;
  for (int k = 0; k < kWords; ++k) d += a[k] > b[k] ? (uint32_t)(a[k] - b[k]) : (uint32_t)(b[k] - a[k]);
  return d;
}

// The whole signature on the host (the hook, and the stand-alone sanitizer program).
inline void signature_host(int rows, int cols, const rebvio_hip_keyline* kl, int n, uint16_t* sig, int* counted_out) {
  uint32_t h[kWords];
  for (int k = 0; k < kWords; ++k) h[k] = 0;
  uint32_t c = 0;
  for (int i = 0; i < n; ++i) {
    const rebvio_hip_keyline& q = kl[i];
    if (!counted(rows, cols, q.pos[0], q.pos[1], q.gradient[0], q.gradient[1], q.gradient_norm)) continue;
    ++h[word_of(rows, cols, q.pos[0], q.pos[1], q.gradient[0], q.gradient[1])];
    ++c;
  }
  for (int k = 0; k < kWords; ++k) sig[k] = normalise(h[k], c);
  *counted_out = (int)c;
}

// The k smallest (distance, index) among rows e < size - exclude_last, ascending, by the kernel's scheme: k rounds of "the
// smallest key above the previous winner". tag 0 in every record.
inline void query_host(const uint16_t* rows384, int size, const uint16_t* sig, int k, int exclude_last, rebvio_hip_place_match* out,
                       int* count) {
  const int eligible = size - exclude_last > 0 ? size - exclude_last : 0;
  const int m = k < eligible ? k : eligible;
  uint64_t lo = 0;
  for (int r = 0; r < m; ++r) {
    uint64_t best = ~(uint64_t)0;
    for (int e = 0; e < eligible; ++e) {
      const uint64_t key = ((uint64_t)distance(rows384 + (size_t)e * kWords, sig) << 32) | (uint32_t)e;
      if (key >= lo && key < best) best = key;
    }
    out[r].distance = (uint32_t)(best >> 32);
    out[r].index = (int32_t)(best & 0xffffffffu);
    out[r].tag = 0;
    lo = best + 1;
  }
  *count = m;
}

}  // namespace plc
}  // namespace rh
