// The per-keyline statement of the depth prior (rebvio_amd/csrc/depth_prior.hpp: dpr::tap and dpr::term - what k_depth_prior and
// rebvio_hip_test_depth_prior_host run) as a stand-alone host program, meant to be built with -fsanitize=address,undefined: no GPU,
// no library, nothing loaded into another process.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I rebvio_amd/csrc
//       tests/cpp/depth_prior_host_check.cpp -o depth_prior_host_check && ./depth_prior_host_check
// Depth images of both formats in heap buffers of EXACTLY the bytes the definition may read - (rows - 1) * pitch + cols * tap size,
// with pitch > width - so a tap one pixel outside the image, or in the padding behind the last row, is caught. Keylines at hostile
// positions: NaN, infinities, 1e30, negative, on and half a pixel around every border; gradients with zero, NaN, negative and
// denormal norms. Checks the outcome word's consistency, that a keyline that is not fused is not written, that a second run gives
// the same bytes, and that every outcome was reached. Prints "ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#include "depth_prior.hpp"

static int fails = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                \
    }                                                         \
  } while (0)

namespace dpr = rh::dpr;

static long seen_none = 0, seen_fused = 0, seen_gated = 0, seen_jump = 0, seen_clamp_lo = 0, seen_clamp_hi = 0, seen_nodir = 0,
            seen_outside_centre = 0, seen_zero_u16 = 0;

static rebvio_hip_depth_prior_opts defaults() {
  rebvio_hip_depth_prior_opts o;
  std::memset(&o, 0, sizeof(o));
  o.tap_px = 2.0; o.jump_rel = 0.1; o.z_min = 0.1; o.z_max = 20.0; o.sigma_z0 = 1e-3; o.sigma_z2 = 2e-3; o.gate_sigma = 3.0;
  o.q_abs = 0.0; o.unit = 0.001;
  return o;
}

struct Kl {
  float px, py, gx, gy, gn, rho, sig;
};

static void run_image(int rows, int cols, int fmt, size_t pad_px, const rebvio_hip_depth_prior_opts& o, std::mt19937& rng) {
  const size_t tb = fmt == REBVIO_HIP_DEPTH_U16 ? 2 : 4, pitch = ((size_t)cols + pad_px) * tb;
  const size_t bytes = (size_t)(rows - 1) * pitch + (size_t)cols * tb;
  std::unique_ptr<char[]> img(new char[bytes]);  // exactly what may be read: the last row has no padding behind it
  std::uniform_real_distribution<double> uz(0.0, 1.0);
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < cols; ++x) {
      const double r = uz(rng);
      // smooth-ish depth with steps, holes, values outside the bounds and (fp32) non-finite ones
      double z = 1.5 + (x > cols / 2 ? 2.0 : 0.0) + 0.01 * y;
      if (r < 0.05) z = 0.0;
      else if (r < 0.08) z = 25.0;
      else if (r < 0.10) z = 0.02;
      else if (r < 0.12) z = 0.03 + 0.02 * uz(rng);
      char* p = img.get() + (size_t)y * pitch + (size_t)x * tb;
      if (fmt == REBVIO_HIP_DEPTH_U16) {
        const uint16_t v = (uint16_t)std::lround(z / o.unit > 65535.0 ? 65535.0 : z / o.unit);
        std::memcpy(p, &v, 2);
      } else {
        float v = (float)z;
        if (r > 0.97) v = std::numeric_limits<float>::quiet_NaN();
        else if (r > 0.96) v = std::numeric_limits<float>::infinity();
        else if (r > 0.95) v = -1.0f;
        std::memcpy(p, &v, 4);
      }
    }
  const dpr::Args a = dpr::make_args(img.get(), pitch, rows, cols, fmt, o);

  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  std::vector<Kl> kls;
  const float xs[] = {nan, inf, -inf, 1e30f, -1e30f, -3.f, -2.5f, -0.5f, -0.50001f, 0.f, 0.49f, 1.5f, (float)cols - 3.f, (float)cols - 2.5f,
                      (float)cols - 1.f, (float)cols - 0.5f, (float)cols - 0.50001f, (float)cols, (float)cols + 1.5f, 2147483648.f,
                      -2147483904.f, 4e9f};
  const float ys[] = {nan, inf, -1e30f, -2.5f, -0.5f, 0.f, 1.5f, (float)rows - 2.5f, (float)rows - 1.f, (float)rows - 0.5f, (float)rows,
                      (float)rows + 1.5f, 3e9f};
  const float gs[][3] = {{1, 0, 1}, {-1, 0, 1}, {0, 1, 1}, {0, -1, 1}, {3, 4, 5}, {1, 1, 0}, {1, 1, nan}, {1, 1, -1}, {inf, 0, 1},
                         {1, 0, 1e-45f}, {nan, nan, 1}, {0, 0, 0}, {1e30f, 1e30f, 1e-30f}};
  for (float x : xs)
    for (float y : ys)
      for (const auto& g : gs) kls.push_back({x, y, g[0], g[1], g[2], 1.0f, 20.0f});
  std::uniform_real_distribution<float> ux(-4.f, (float)cols + 4.f), uy(-4.f, (float)rows + 4.f), ur(1e-3f, 3.f), us(0.f, 1.f), ug(-9.f, 9.f);
  for (int k = 0; k < 4000; ++k) {
    const float gx = ug(rng), gy = ug(rng);
    kls.push_back({ux(rng), uy(rng), gx, gy, std::sqrt(gx * gx + gy * gy), ur(rng), k % 7 == 0 ? 0.f : us(rng) * us(rng)});
  }
  for (const Kl& k : kls) {
    const float canary_r = -7.f, canary_s = -9.f;
    float rho_n = canary_r, sig_n = canary_s, rho_2 = canary_r, sig_2 = canary_s;
    const int oc = dpr::term(a, k.px, k.py, k.gx, k.gy, k.gn, k.rho, k.sig, &rho_n, &sig_n);
    const int oc2 = dpr::term(a, k.px, k.py, k.gx, k.gy, k.gn, k.rho, k.sig, &rho_2, &sig_2);
    CHECK(oc == oc2 && std::memcmp(&rho_n, &rho_2, 4) == 0 && std::memcmp(&sig_n, &sig_2, 4) == 0);
    const int base = oc & 3;
    CHECK((oc & ~(3 | dpr::kJumpBit | dpr::kClampedBit)) == 0 && base != 3);
    if (base == dpr::kNone) CHECK(oc == 0);
    if (base != dpr::kFused) {
      CHECK(!(oc & dpr::kClampedBit));
      CHECK(rho_n == canary_r && sig_n == canary_s);  // not written
    } else {
      CHECK(std::isfinite(rho_n) && std::isfinite(sig_n) && sig_n >= 0.f);
      CHECK(rho_n >= rh::kfp::kRhoMin && rho_n <= rh::kfp::kRhoMax);
      if (oc & dpr::kClampedBit) (rho_n == rh::kfp::kRhoMin ? seen_clamp_lo : seen_clamp_hi)++;
    }
    // the centre tap of a keyline that lies outside, or at a bad position, does not exist
    double z;
    const bool centre = dpr::tap(a, (double)k.px, (double)k.py, &z);
    if (!(k.px + 0.5 >= 0.0 && k.px + 0.5 < cols && k.py + 0.5 >= 0.0 && k.py + 0.5 < rows)) {
      CHECK(!centre);
      ++seen_outside_centre;
    } else if (centre) {
      CHECK(z >= o.z_min && z <= o.z_max);
    } else if (fmt == REBVIO_HIP_DEPTH_U16) {
      ++seen_zero_u16;
    }
    const bool dir = k.gn > 0.f && std::isfinite((double)k.gx / (double)k.gn) && std::isfinite((double)k.gy / (double)k.gn);
    if (!dir) {
      ++seen_nodir;
      CHECK((base != dpr::kNone) == centre);  // the centre tap alone decides
      CHECK(!(oc & dpr::kJumpBit));           // one tap cannot jump
    }
    seen_none += base == dpr::kNone;
    seen_fused += base == dpr::kFused;
    seen_gated += base == dpr::kGated;
    seen_jump += (oc & dpr::kJumpBit) != 0;
  }
}

int main() {
  std::mt19937 rng(5150);
  const rebvio_hip_depth_prior_opts d = defaults();
  rebvio_hip_depth_prior_opts wide = d;  // lets depths through that clamp on both sides
  wide.z_min = 0.01;
  wide.z_max = 5000.0;
  wide.unit = 0.1;
  for (int fmt : {REBVIO_HIP_DEPTH_U16, REBVIO_HIP_DEPTH_F32})
    for (size_t pad : {(size_t)0, (size_t)1, (size_t)5}) {
      run_image(32, 32, fmt, pad, d, rng);
      run_image(33, 37, fmt, pad, d, rng);
      run_image(33, 37, fmt, pad, wide, rng);
      rebvio_hip_depth_prior_opts t0 = d;
      t0.tap_px = 0.0;
      t0.q_abs = 0.5;
      run_image(32, 35, fmt, pad, t0, rng);
    }
  // the low clamp needs a depth above 1000 m
  {
    std::unique_ptr<float[]> img(new float[32 * 32]);
    for (int i = 0; i < 32 * 32; ++i) img[i] = 2000.0f;
    const dpr::Args a = dpr::make_args(img.get(), 32 * 4, 32, 32, REBVIO_HIP_DEPTH_F32, wide);
    float r = 0, s = 0;
    const int oc = dpr::term(a, 5.f, 5.f, 1.f, 0.f, 1.f, 1.0f, 20.0f, &r, &s);
    CHECK(oc == (dpr::kFused | dpr::kClampedBit) && r == rh::kfp::kRhoMin);
    ++seen_clamp_lo;
  }
  std::printf("none %ld fused %ld gated %ld jump %ld clamp_lo %ld clamp_hi %ld nodir %ld outside %ld zero_u16 %ld\n", seen_none, seen_fused,
              seen_gated, seen_jump, seen_clamp_lo, seen_clamp_hi, seen_nodir, seen_outside_centre, seen_zero_u16);
  CHECK(seen_none > 0 && seen_fused > 0 && seen_gated > 0 && seen_jump > 0 && seen_clamp_lo > 0 && seen_clamp_hi > 0 && seen_nodir > 0 &&
        seen_outside_centre > 0 && seen_zero_u16 > 0);
  if (fails) {
    std::printf("%d checks failed\n", fails);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
