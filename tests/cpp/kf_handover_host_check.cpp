// The host side of rebvio_hip_kf_snapshot_handover_depth (rebvio_amd/csrc/kf_handover.hpp: kfp::handover_claim_term,
// kfp::handover_apply_term and the two passes in index order, kfp::handover_host - what rebvio_hip_test_kf_handover_host runs) as a
// stand-alone host program, meant to be built with -fsanitize=address,undefined: no GPU, no library, nothing loaded into another
// process.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I rebvio_amd/csrc
//       tests/cpp/kf_handover_host_check.cpp -o kf_handover_host_check && ./kf_handover_host_check
// Seeded random distance fields (ids with empty cells, ids beyond the successor's size, distances) over random keylines, outgoing
// snapshots of 0 .. 600 keylines and successors of 0 .. n_cur slots with NaN, infinite, denormal, huge and out-of-frame values planted
// in every field, all in heap buffers of exactly the needed size (a read or write past a snapshot, a keyline array, the field or the
// scratch is caught). Checks the bookkeeping identities, the association words against the counts, that src is untouched, that a slot
// changes only where it was adopted and never grows its sigma, that a second run gives the same bytes, and that every outcome was
// reached. Prints "ok".
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#include "kf_handover.hpp"

static int fails = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                \
    }                                                         \
  } while (0)

// memcmp == 0, with empty ranges equal (a vector of size 0 may hand out a null pointer)
static bool same_bytes(const void* a, const void* b, size_t bytes) { return bytes == 0 || std::memcmp(a, b, bytes) == 0; }

int main() {
  std::mt19937 rng(8642);
  std::uniform_real_distribution<float> uni(0.0f, 1.0f);
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float special[] = {nan, inf, -inf, 0.0f, -0.0f, std::numeric_limits<float>::denorm_min(), std::numeric_limits<float>::max(),
                           -std::numeric_limits<float>::max(), 1e30f, -1e30f, 1e6f, -1e6f};
  const int n_special = (int)(sizeof(special) / sizeof(special[0]));
  long seen_assoc = 0, seen_range = 0, seen_adopted = 0, seen_kept = 0, seen_conflict = 0, seen_losers = 0, seen_beyond = 0;
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
      // the successor: all of the map's keylines, fewer (ids beyond its size), or none
      const int m = field % 4 == 0 ? n_cur / 2 : field % 9 == 5 ? 0 : n_cur;
      // exactly n outgoing keylines and m slots on the heap
      std::unique_ptr<float[]> prs4(new float[4 * (size_t)n + (n == 0)]), nrm(new float[2 * (size_t)n + (n == 0)]);
      std::unique_ptr<unsigned[]> mt(new unsigned[(size_t)n + (n == 0)]);
      std::unique_ptr<float[]> dp(new float[4 * (size_t)m + (m == 0)]), dp2(new float[4 * (size_t)m + (m == 0)]);
      std::unique_ptr<unsigned[]> dm(new unsigned[(size_t)m + (m == 0)]), dm2(new unsigned[(size_t)m + (m == 0)]);
      for (int j = 0; j < n; ++j) {
        prs4[4 * j] = 1.4f * cols * (uni(rng) - 0.5f);  // some project out of the frame
        prs4[4 * j + 1] = 1.4f * rows * (uni(rng) - 0.5f);
        prs4[4 * j + 2] = std::exp(-3.0f + 4.0f * uni(rng));
        prs4[4 * j + 3] = 0.3f * prs4[4 * j + 2] * uni(rng);
        if (rng() % 5u == 0) prs4[4 * j + 3] = 0.05f * prs4[4 * j + 2];  // equal sigmas among claimants of one slot
        mt[j] = rng() % 6u;
        const float a = 6.2831853f * uni(rng);
        nrm[2 * j] = std::cos(a);
        nrm[2 * j + 1] = std::sin(a);
        if (field % 2 == 1 && rng() % 4u == 0) prs4[4 * j + (int)(rng() % 4u)] = special[rng() % (unsigned)n_special];
        if (field % 2 == 1 && rng() % 9u == 0) nrm[2 * j + (int)(rng() % 2u)] = special[rng() % (unsigned)n_special];
      }
      for (int i = 0; i < m; ++i) {
        dp[4 * i] = cols * uni(rng);
        dp[4 * i + 1] = rows * uni(rng);
        dp[4 * i + 2] = std::exp(-3.0f + 4.0f * uni(rng));
        dp[4 * i + 3] = dp[4 * i + 2] * (rng() % 3u == 0 ? 0.001f : 2.0f * uni(rng));
        dm[i] = rng() % 6u;
        if (field % 2 == 1 && rng() % 6u == 0) dp[4 * i + 2 + (int)(rng() % 2u)] = special[rng() % (unsigned)n_special];
      }
      std::memcpy(dp2.get(), dp.get(), 4 * (size_t)m * sizeof(float));
      std::memcpy(dm2.get(), dm.get(), (size_t)m * sizeof(unsigned));
      const std::vector<float> src_before(prs4.get(), prs4.get() + 4 * (size_t)n), dst_before(dp.get(), dp.get() + 4 * (size_t)m);
      const std::vector<unsigned> mt_before(mt.get(), mt.get() + n), dm_before(dm.get(), dm.get() + m);
      rebvio_hip_kf_handover_opts o;
      std::memset(&o, 0, sizeof(o));
      o.kf_filter = {field % 4 == 0 ? 0u : 2u, field % 4 == 1 ? 1e9f : 0.5f, 1e-3f, 20.0f};
      o.min_cos = field % 6 == 0 ? -1.0 : 0.5;
      o.gate_sigma = field % 5 == 0 ? 0.3 : 3.0;
      o.q_abs = field % 7 == 3 ? 1e200 : field % 7 == 4 ? 0.01 : 0.0;
      o.max_dist = 11 - field % 4;
      const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0.01 * (field % 3), -0.02, field % 5 == 1 ? -0.9 : 0.03 * (field % 2)};
      rebvio_hip_kf_handover res, again;
      std::unique_ptr<unsigned long long[]> key(new unsigned long long[(size_t)m + (m == 0)]);
      std::unique_ptr<rh::kfp::HandoverStage[]> stage(new rh::kfp::HandoverStage[(size_t)n + (n == 0)]);
      std::unique_ptr<int[]> assoc(new int[(size_t)n + (n == 0)]), assoc2(new int[(size_t)n + (n == 0)]);
      const float* normals = field % 4 == 3 ? nullptr : nrm.get();
      rh::kfp::handover_host(am, prs4.get(), mt.get(), normals, n, dp.get(), dm.get(), m, o, I, t, key.get(), stage.get(), assoc.get(), &res);
      rh::kfp::handover_host(am, prs4.get(), mt.get(), normals, n, dp2.get(), dm2.get(), m, o, I, t, key.get(), stage.get(), assoc2.get(), &again);
      CHECK(std::memcmp(&res, &again, sizeof(res)) == 0 && same_bytes(assoc.get(), assoc2.get(), (size_t)n * sizeof(int)));
      CHECK(same_bytes(dp.get(), dp2.get(), 4 * (size_t)m * sizeof(float)) && same_bytes(dm.get(), dm2.get(), (size_t)m * sizeof(unsigned)));
      CHECK(same_bytes(prs4.get(), src_before.data(), 4 * (size_t)n * sizeof(float)));  // src is never written
      CHECK(same_bytes(mt.get(), mt_before.data(), (size_t)n * sizeof(unsigned)));
      CHECK(res.candidates == n && res.associated >= 0 && res.associated <= n && res.out_of_range >= 0 && res.claimed <= m);
      CHECK(res.claimed == res.adopted + res.kept + res.conflicts && res.adopted >= 0 && res.kept >= 0 && res.conflicts >= 0);
      CHECK(res.associated - res.out_of_range - res.claimed >= 0);
      int n_none = 0, n_adopted = 0;
      std::vector<char> adopted((size_t)m, 0);
      for (int j = 0; j < n; ++j) {
        const int v = assoc[j];
        CHECK(v == INT_MIN || (v >= -m && v < m));
        n_none += v == INT_MIN;
        if (v >= 0) {
          ++n_adopted;
          CHECK(!adopted[(size_t)v]);  // one winner per slot
          adopted[(size_t)v] = 1;
        }
      }
      CHECK(n_none == n - res.associated && n_adopted == res.adopted);
      for (int i = 0; i < m; ++i) {
        const bool same = std::memcmp(dp.get() + 4 * i, dst_before.data() + 4 * (size_t)i, 4 * sizeof(float)) == 0 && dm[i] == dm_before[(size_t)i];
        if (!adopted[(size_t)i]) {
          CHECK(same);  // a slot that is not adopted keeps all its bits
          continue;
        }
        CHECK(std::memcmp(dp.get() + 4 * i, dst_before.data() + 4 * (size_t)i, 2 * sizeof(float)) == 0);  // pos_img is never written
        CHECK(dp[4 * i + 3] < dst_before[4 * (size_t)i + 3] && dp[4 * i + 2] >= 1e-3f && dp[4 * i + 2] <= 20.0f && dm[i] >= dm_before[(size_t)i]);
      }
      if (m < n_cur)
        for (int j = 0; j < n; ++j) seen_beyond += assoc[j] == INT_MIN;
      seen_assoc += res.associated;
      seen_range += res.out_of_range;
      seen_adopted += res.adopted;
      seen_kept += res.kept;
      seen_conflict += res.conflicts;
      seen_losers += res.associated - res.out_of_range - res.claimed;
    }
  }
  std::printf("associated %ld out_of_range %ld adopted %ld kept %ld conflicts %ld losers %ld\n", seen_assoc, seen_range, seen_adopted, seen_kept,
              seen_conflict, seen_losers);
  CHECK(seen_assoc > 2000 && seen_range > 0 && seen_adopted > 0 && seen_kept > 0 && seen_conflict > 0 && seen_losers > 0 && seen_beyond > 0);
  if (fails == 0) std::printf("ok\n");
  return fails ? 1 : 0;
}
