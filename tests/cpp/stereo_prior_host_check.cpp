// The statements of the stereo prior (rebvio_amd/csrc/stereo_prior.hpp: spr::left_setup, fold_candidate, decide, update - what
// k_stereo_prior and rebvio_hip_test_stereo_prior_host run) as a stand-alone host program, meant to be built with
// -fsanitize=address,undefined: no GPU, no library, nothing loaded into another process.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I rebvio_amd/csrc
//       tests/cpp/stereo_prior_host_check.cpp -o stereo_prior_host_check && ./stereo_prior_host_check
// The right map's mask and keyline table sit in heap buffers of EXACTLY the bytes the definition may read - rows * cols ints and
// nr keylines - so a window cell one column or one row outside the image, or a gather behind the table, is caught; the mask holds
// words behind the table's end and below -1, which are no keyline. Left keylines at hostile positions: NaN, infinities, 1e30,
// negative, on and around every border; gradients with zero, NaN, negative and denormal norms. The window is walked twice, row by
// row and as 16 lanes would (columns lane, lane + 16, ... per lane, the lanes' folds joined in a butterfly), and both walks must
// agree in every bit. Checks the outcome word's consistency, that a keyline that is not fused is not written, and that every
// outcome was reached. Prints "ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#include "stereo_prior.hpp"

static int fails = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                \
    }                                                         \
  } while (0)

namespace spr = rh::spr;

static long seen_oc[5] = {0, 0, 0, 0, 0}, seen_clamp_lo = 0, seen_clamp_hi = 0, seen_clipped_away = 0, seen_stray_word = 0;

static rebvio_hip_stereo_prior_opts defaults(double baseline) {
  rebvio_hip_stereo_prior_opts o;
  std::memset(&o, 0, sizeof(o));
  o.baseline = baseline; o.d_min = 0.0; o.d_max = 64.0; o.min_ux = 0.5; o.row_tol = 1; o.sigma_px = 0.5; o.gate_sigma = 3.0;
  o.ambig_px = 2.0; o.cos_min = std::cos(M_PI / 4); o.norm_tol = 1.0; o.q_abs = 0.0;
  return o;
}

struct Kl {
  float px, py, gx, gy, gn, rho, sig;
};

struct Right {
  int rows, cols, nr;
  std::unique_ptr<int[]> mask;  // exactly rows * cols
  std::unique_ptr<Kl[]> kl;     // exactly nr
};

// one keyline through the statements; lanes = 0: row by row, else as `lanes` lanes and a butterfly
static int run_one(const spr::Args& a, const Right& R, const Kl& k, int lanes, float* rho_out, float* sig_out, int* win) {
  spr::Left L;
  int oc = spr::left_setup(a, k.px, k.py, k.gx, k.gy, k.gn, k.rho, k.sig, &L);
  *win = -1;
  if (oc >= 0) return oc;
  if (L.x0 > L.x1) ++seen_clipped_away;
  std::vector<spr::Fold> f(lanes ? lanes : 1);
  for (auto& x : f) spr::fold_clear(&x);
  for (int t = 0; t < (a.row_tol ? 3 : 1); ++t) {
    const int y = L.yi + (t == 0 ? 0 : (t == 1 ? -1 : 1));
    if (y < 0 || y >= R.rows) continue;
    const int* row = R.mask.get() + (size_t)y * R.cols;
    for (int x = L.x0; x <= L.x1; ++x) {
      const int j = row[x];
      if (j < 0 || j >= R.nr) {
        seen_stray_word += j != -1;
        continue;
      }
      const Kl& q = R.kl[j];
      spr::fold_candidate(a, L, j, q.px, q.py, q.gx, q.gy, q.gn, &f[lanes ? (x - L.x0) % lanes : 0]);
    }
  }
  for (int o = lanes / 2; o > 0; o >>= 1) {
    const std::vector<spr::Fold> was = f;
    for (int l = 0; l < lanes; ++l) spr::fold_join(&f[l], was[l ^ o]);
  }
  oc = spr::decide(a, f[0]);
  if (oc >= 0) return oc;
  oc = spr::update(a, L, f[0].d_win, rho_out, sig_out);
  if ((oc & 7) == spr::kFused) *win = f[0].j;
  return oc;
}

static void run_map(int rows, int cols, float fm, const rebvio_hip_stereo_prior_opts& o, double fill, std::mt19937& rng) {
  Right R;
  R.rows = rows;
  R.cols = cols;
  R.mask.reset(new int[(size_t)rows * cols]);
  std::uniform_real_distribution<double> u01(0.0, 1.0);
  std::vector<Kl> rk;
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < cols; ++x) {
      int& w = R.mask[(size_t)y * cols + x];
      w = -1;
      const double r = u01(rng);
      if (r < fill) {
        w = (int)rk.size();
        float gx = (float)(8.0 * u01(rng) - 2.0), gy = (float)(6.0 * u01(rng) - 3.0);
        float gn = std::sqrt(gx * gx + gy * gy);
        float px = (float)(x + u01(rng) - 0.5), py = (float)(y + u01(rng) - 0.5);
        const double s = u01(rng);
        if (s < 0.01) gn = 0.f;
        else if (s < 0.02) gn = nan;
        else if (s < 0.03) px = nan;
        else if (s < 0.04) gx = inf;
        else if (s < 0.05) py = -inf;
        else if (s < 0.06) gn = 1e-45f;
        rk.push_back({px, py, gx, gy, gn, 1.f, 1.f});
      } else if (r < fill + 0.01) {
        w = -2 - (int)(1000 * u01(rng));  // below -1
      } else if (r < fill + 0.02) {
        w = 0x7fffffff - (int)(1000 * u01(rng));  // far behind the table
      }
    }
  R.nr = (int)rk.size();
  // ... and words just behind the table's end
  for (int k = 0; k < 8; ++k) R.mask[(size_t)(u01(rng) * rows * cols) % ((size_t)rows * cols)] = R.nr + k / 4;
  R.kl.reset(new Kl[rk.size()]);
  for (size_t k = 0; k < rk.size(); ++k) R.kl[k] = rk[k];
  const spr::Args a = spr::make_args(rows, cols, fm, o);

  std::vector<Kl> kls;
  const float xs[] = {nan, inf, -inf, 1e30f, -1e30f, -3.f, -0.5f, -0.50001f, 0.f, 0.49f, 1.5f, 2.f, (float)cols - 1.f, (float)cols - 0.5f,
                      (float)cols - 0.50001f, (float)cols, (float)cols + 1.5f, 2147483648.f, -2147483904.f, 4e9f};
  const float ys[] = {nan, inf, -1e30f, -0.5f, -0.50001f, 0.f, 1.f, (float)rows - 2.f, (float)rows - 1.f, (float)rows - 0.5f, (float)rows, 3e9f};
  const float gs[][3] = {{1, 0, 1}, {-1, 0, 1}, {0, 1, 1}, {3, 4, 5}, {4, 3, 5}, {1, 1, 0}, {1, 1, nan}, {1, 1, -1}, {inf, 0, 1},
                         {1, 0, 1e-45f}, {nan, nan, 1}, {0, 0, 0}, {1e30f, 1e30f, 1e-30f}};
  for (float x : xs)
    for (float y : ys)
      for (const auto& g : gs) kls.push_back({x, y, g[0], g[1], g[2], 1.0f, 20.0f});
  std::uniform_real_distribution<float> ur(1e-3f, 3.f), us(0.f, 1.f), ud(0.f, 30.f);
  for (int k = 0; k < 4000 && R.nr > 0; ++k) {  // a right keyline moved by a disparity, its gradient disturbed
    const Kl& q = R.kl[(size_t)(u01(rng) * R.nr) % R.nr];
    const float d = ud(rng);
    const float gx = q.gx * (0.8f + 0.4f * us(rng)), gy = q.gy + 0.3f * (us(rng) - 0.5f);
    const int kind = k % 4;
    kls.push_back({q.px + d, q.py + (float)(k % 3 - 1) * (k % 5 == 0), gx, gy, std::sqrt(gx * gx + gy * gy),
                   kind == 0 ? 1.f : (kind == 1 ? (float)(d / a.fb) : ur(rng)), kind == 0 ? 20.f : (kind == 1 ? 0.05f * us(rng) : us(rng) * us(rng))});
  }
  for (const Kl& k : kls) {
    const float canary_r = -7.f, canary_s = -9.f;
    float rho_n = canary_r, sig_n = canary_s, rho_2 = canary_r, sig_2 = canary_s;
    int win = 0, win2 = 0;
    const int oc = run_one(a, R, k, 0, &rho_n, &sig_n, &win);
    const int oc2 = run_one(a, R, k, 16, &rho_2, &sig_2, &win2);
    CHECK(oc == oc2 && win == win2 && std::memcmp(&rho_n, &rho_2, 4) == 0 && std::memcmp(&sig_n, &sig_2, 4) == 0);
    const int base = oc & 7;
    CHECK((oc & ~(7 | spr::kClampedBit)) == 0 && base <= 4);
    if (base != spr::kFused) {
      CHECK(oc == base && win == -1);
      CHECK(rho_n == canary_r && sig_n == canary_s);  // not written
    } else {
      CHECK(win >= 0 && win < R.nr);
      CHECK(std::isfinite(rho_n) && std::isfinite(sig_n) && sig_n >= 0.f);
      CHECK(rho_n >= rh::kfp::kRhoMin && rho_n <= rh::kfp::kRhoMax);
      if (oc & spr::kClampedBit) (rho_n == rh::kfp::kRhoMin ? seen_clamp_lo : seen_clamp_hi)++;
    }
    const bool dir = k.gn > 0.f && std::isfinite((double)k.gx / (double)k.gn) && std::isfinite((double)k.gy / (double)k.gn) &&
                     std::fabs((double)k.gx / (double)k.gn) >= o.min_ux;
    CHECK((base == spr::kUnusable) == !dir);
    if (dir && !(k.px + 0.5 >= 0.0 && k.px + 0.5 < cols && k.py + 0.5 >= 0.0 && k.py + 0.5 < rows)) CHECK(oc == spr::kNone);
    ++seen_oc[base];
  }
}

int main() {
  std::mt19937 rng(5151);
  const rebvio_hip_stereo_prior_opts d = defaults(0.125);
  for (double fill : {0.0, 0.05, 0.3, 1.0}) {
    run_map(32, 80, 80.f, d, fill, rng);
    rebvio_hip_stereo_prior_opts s = d;
    s.d_max = 37.0;
    run_map(33, 37, 80.f, s, fill, rng);
    s.d_min = 3.0;
    s.d_max = 9.5;
    s.row_tol = 0;
    s.q_abs = 0.5;
    s.ambig_px = 0.5;
    run_map(33, 37, 80.f, s, fill, rng);
    s.d_min = s.d_max = 36.0;  // most windows clipped to nothing
    run_map(33, 37, 80.f, s, fill, rng);
    rebvio_hip_stereo_prior_opts one = d;  // an image of one pixel
    one.d_max = 1.0;
    run_map(1, 1, 80.f, one, fill, rng);
    run_map(48, 96, 80.f, defaults(0.00125), fill, rng);  // rho_m far above RHO_MAX
    run_map(48, 96, 80.f, defaults(125.0), fill, rng);    // ... and below RHO_MIN
  }
  std::printf("none %ld fused %ld gated %ld unusable %ld ambiguous %ld clamp_lo %ld clamp_hi %ld clipped_away %ld stray_words %ld\n", seen_oc[0],
              seen_oc[1], seen_oc[2], seen_oc[3], seen_oc[4], seen_clamp_lo, seen_clamp_hi, seen_clipped_away, seen_stray_word);
  CHECK(seen_oc[0] > 0 && seen_oc[1] > 0 && seen_oc[2] > 0 && seen_oc[3] > 0 && seen_oc[4] > 0 && seen_clamp_lo > 0 && seen_clamp_hi > 0 &&
        seen_clipped_away > 0 && seen_stray_word > 0);
  if (fails) {
    std::printf("%d checks failed\n", fails);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
