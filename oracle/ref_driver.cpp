/*
 * ref_driver.cpp - a C ABI over the reference's own public classes (TEST INFRASTRUCTURE, NOT PRODUCT CODE).
 *
 * Compiled by `make -C oracle ref` together with the reference's scale_space.cpp, edge_detector.cpp, edge_map.cpp and core.cpp
 * (read in place from the reference checkout, unmodified) into oracle/_ref/librebvio_ref.so. Everything here is a call into
 * those classes; nothing of the hot path is restated. The functions mirror the subset of rebvio_oracle.h that the public
 * classes can serve, with the prefix ref_ and the oracle's record layouts (orc_keyline, orc_params), so that a test can drive
 * both libraries with the same code (oracle/ref_py.py).
 *
 * What the public interface does not reach, and how it is dealt with:
 *  - Core's DistanceField is private: ref_distance_field reads a DistanceField of its own, built from the same map with the
 *    same search range (the class is public, core.hpp).
 *  - ScaleSpace's two scale images are private: ref_scale_space smooths the image with two FastGaussian objects constructed
 *    with the arguments ScaleSpace's constructor gives its own.
 *  - EdgeDetector's dense mask and auto threshold are private: the map's own mask() and threshold() carry the same values.
 *  - Core::testfk is declared inline and defined in core.cpp only: it cannot be called from another unit and is reached
 *    through calculatefJ.
 *  - EdgeMapConfig is fixed at its defaults for every map EdgeDetector makes; minimizeVel reports neither its accept mask nor
 *    its quantile; extRotVel does not report JtF.
 *  - the detector's plane-fit pseudo-inverse is a function-local static: first use fixes it for the process (its size is a
 *    compile-time constant of the reference, so every context of a process wants the same one).
 */
#include <rebvio/core.hpp>
#include <rebvio/edge_detector.hpp>
#include <rebvio/sab_estimator.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "rebvio_oracle.h"

using rebvio::types::KeyLine;

static_assert(sizeof(KeyLine) == sizeof(orc_keyline), "orc_keyline is the reference's KeyLine, field for field");
static_assert(sizeof(KeyLine) == 84, "KeyLine is 84 bytes");

// Core::estimateBias (inertial glue, never called through this library) constructs a SABEstimator; sab_estimator.cpp is not part
// of the library, so the members core.cpp refers to are given definitions that end the process.
namespace rebvio {
static void no_sab() {
  std::fputs("oracle/ref_driver: SABEstimator is not part of librebvio_ref\n", stderr);
  std::abort();
}
SABEstimator::SABEstimator(SABEstimator::Config& _config) : config_(_config) { no_sab(); }
SABEstimator::~SABEstimator() {}
bool SABEstimator::problem(types::Matrix7f&, types::Vector7f&, const types::Vector7f&) { no_sab(); return false; }
int SABEstimator::gaussNewton(types::Vector7f&, int, types::Float, types::Float) { no_sab(); return 0; }
}  // namespace rebvio

struct ref_ctx {
  orc_params p;
  rebvio::Camera::SharedPtr cam;
  rebvio::EdgeDetectorConfig::SharedPtr dcfg;
  rebvio::CoreConfig::SharedPtr ccfg;
  std::unique_ptr<rebvio::EdgeDetector> det;
  std::unique_ptr<rebvio::ScaleSpace> ss;
  std::unique_ptr<rebvio::FastGaussian> g0, g1;
  std::unique_ptr<rebvio::Core> core;
  std::unique_ptr<rebvio::DistanceField> df;
};
struct ref_map {
  rebvio::EdgeMap::SharedPtr m;
};

namespace {
KeyLine from_record(const orc_keyline& k) {
  rebvio::types::Point2Df a = TooN::Zeros;
  rebvio::types::Vector2f g = TooN::Zeros;
  KeyLine out(a, g, rebvio::types::Point2Df(TooN::Zeros));
  std::memcpy(static_cast<void*>(&out), &k, sizeof(k));
  return out;
}
rebvio::types::Vector3f vec3(const float* v) { return TooN::makeVector(v[0], v[1], v[2]); }
rebvio::types::Matrix3f mat3(const float* m) {
  rebvio::types::Matrix3f r;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r(i, j) = m[i * 3 + j];
  return r;
}
cv::Mat image(const ref_ctx* c, const float* img) {
  cv::Mat m(c->p.rows, c->p.cols, CV_32FC1);
  for (int r = 0; r < c->p.rows; ++r) std::memcpy(m.ptr<float>(r), img + (size_t)r * c->p.cols, sizeof(float) * c->p.cols);
  return m;
}
void image_out(const ref_ctx* c, const cv::Mat& m, float* out) {
  if (!out) return;
  for (int r = 0; r < c->p.rows; ++r) std::memcpy(out + (size_t)r * c->p.cols, m.ptr<float>(r), sizeof(float) * c->p.cols);
}
}  // namespace

extern "C" {

ref_ctx* ref_create(const orc_params* p) {
  ref_ctx* c = new ref_ctx;
  c->p = *p;
  c->cam = std::make_shared<rebvio::Camera>();
  c->cam->rows_ = p->rows;
  c->cam->cols_ = p->cols;
  c->cam->fx_ = c->cam->fy_ = c->cam->fm_ = p->fm;
  c->cam->cx_ = p->cx;
  c->cam->cy_ = p->cy;
  c->dcfg = std::make_shared<rebvio::EdgeDetectorConfig>();
  c->dcfg->keylines_ref = p->keylines_ref;
  c->dcfg->keylines_max = p->keylines_max;
  c->dcfg->pos_neg_threshold = p->pos_neg_threshold;
  c->dcfg->dog_threshold = p->dog_threshold;
  c->dcfg->threshold = p->threshold;
  c->dcfg->gain = p->gain;
  c->dcfg->max_threshold = p->max_threshold;
  c->dcfg->min_threshold = p->min_threshold;
  c->ccfg = std::make_shared<rebvio::CoreConfig>();
  c->ccfg->search_range = p->search_range;
  c->ccfg->reweight_distance = p->reweight_distance;
  c->ccfg->match_treshold = p->match_treshold;
  c->ccfg->min_match_threshold = p->min_match_threshold;
  c->ccfg->iterations = p->iterations;
  c->ccfg->global_min_matches_threshold = p->global_min_matches_threshold;
  c->ccfg->pixel_uncertainty = p->pixel_uncertainty;
  c->ccfg->quantile_cutoff = p->quantile_cutoff;
  c->ccfg->quantile_num_bins = p->quantile_num_bins;
  c->ccfg->reshape_q_abs = p->reshape_q_abs;
  c->det.reset(new rebvio::EdgeDetector(c->cam, c->dcfg));
  c->ss.reset(new rebvio::ScaleSpace(c->cam));
  c->g0.reset(new rebvio::FastGaussian(c->cam, 3.56359, 3));                       // as ScaleSpace's constructor
  c->g1.reset(new rebvio::FastGaussian(c->cam, c->g0->sigma_true_ * 1.2599, 3));   // constructs its two filters
  c->core.reset(new rebvio::Core(c->cam, c->ccfg));
  c->df.reset(new rebvio::DistanceField(p->rows, p->cols, p->search_range));
  return c;
}
void ref_destroy(ref_ctx* c) { delete c; }

/* ---- scale space ---- */
void ref_scale_space(ref_ctx* c, const float* img, float* scale0, float* scale1, float* dog, float* mag) {
  cv::Mat in = image(c, img);
  c->ss->build(in);
  image_out(c, c->ss->dog(), dog);
  image_out(c, c->ss->mag(), mag);
  if (scale0) image_out(c, c->g0->smooth(in), scale0);
  if (scale1) image_out(c, c->g1->smooth(in), scale1);
}
int ref_filter_width(ref_ctx* c, int filter, int pass) { return (filter ? c->g1 : c->g0)->widths_[pass]; }
void ref_smooth_n(ref_ctx* c, const float* img, float sigma, int n, float* out, int* widths_out) {
  rebvio::FastGaussian f(c->cam, sigma, n);
  cv::Mat in = image(c, img);
  image_out(c, f.smooth(in), out);
  for (int i = 0; i < n; ++i) widths_out[i] = f.widths_[i];
}

/* ---- detection ---- */
ref_map* ref_detect(ref_ctx* c, const float* img, uint64_t ts_us) {
  rebvio::types::Image im{ts_us, image(c, img)};
  return new ref_map{c->det->detect(im)};
}
float ref_detector_threshold(ref_ctx* c) { return c->dcfg->threshold; }

/* ---- maps ---- */
int ref_map_size(ref_map* m) { return m->m->size(); }
float ref_map_threshold(ref_map* m) { return m->m->threshold(); }
void ref_map_set_threshold(ref_map* m, float t) { m->m->threshold(t); }
void ref_map_get_keylines(ref_map* m, orc_keyline* out) {
  if (m->m->size()) std::memcpy(out, static_cast<const void*>(m->m->keylines().data()), sizeof(orc_keyline) * m->m->size());
}
void ref_map_set_keylines(ref_map* m, const orc_keyline* in, int n) {
  std::vector<KeyLine>& kl = m->m->keylines();
  kl.clear();
  for (int i = 0; i < n; ++i) kl.push_back(from_record(in[i]));
}
void ref_map_get_mask(ref_ctx* c, ref_map* m, int* mask_out) { /* dense rows*cols, -1 = none */
  const int n = c->p.rows * c->p.cols;
  for (int i = 0; i < n; ++i) mask_out[i] = -1;
  for (const auto& kv : m->m->mask())
    if ((int)kv.first < n) mask_out[kv.first] = (int)kv.second;
}
ref_map* ref_map_clone(ref_map* m) { return new ref_map{std::make_shared<rebvio::EdgeMap>(*m->m)}; }
void ref_map_free(ref_map* m) { delete m; }

/* ---- distance field ---- */
void ref_build_distance_field(ref_ctx* c, ref_map* m) {
  c->core->buildDistanceField(m->m);
  c->df->build(m->m);
}
void ref_distance_field(ref_ctx* c, int* id_out, int* dist_out) {
  const int n = c->p.rows * c->p.cols;
  for (int i = 0; i < n; ++i) {
    id_out[i] = (*c->df)[i].id;
    dist_out[i] = (*c->df)[i].distance;
  }
}

/* ---- tracking ---- */
void ref_rotate_keylines(ref_ctx*, ref_map* m, const float R[9]) { m->m->rotateKeylines(mat3(R)); }
float ref_estimate_quantile(ref_map* m, float percentile, int num_bins) { return m->m->estimateQuantile(percentile, num_bins); }
float ref_try_vel(ref_ctx* c, ref_map* m, const float vel[3], float sigma_rho_min, float* residuals, float JtJ[9], float JtF[3]) {
  rebvio::types::Matrix3f A;
  rebvio::types::Vector3f b;
  const float s = c->core->tryVel(m->m, A, b, vec3(vel), sigma_rho_min, residuals);
  for (int i = 0; i < 3; ++i) {
    JtF[i] = b[i];
    for (int j = 0; j < 3; ++j) JtJ[i * 3 + j] = A(i, j);
  }
  return s;
}
float ref_minimize_vel(ref_ctx* c, ref_map* m, float vel[3], float Rvel[9]) {
  rebvio::types::Vector3f v = vec3(vel);
  rebvio::types::Matrix3f R = TooN::Zeros;
  const float F = c->core->minimizeVel(m->m, v, R);
  for (int i = 0; i < 3; ++i) {
    vel[i] = v[i];
    for (int j = 0; j < 3; ++j) Rvel[i * 3 + j] = R(i, j);
  }
  return F;
}
int ref_forward_match(ref_map* old_map, ref_map* new_map) { return old_map->m->forwardMatch(new_map->m); }
int ref_ext_rot_vel(ref_ctx* c, ref_map* m, const float vel[3], float Wx[36], float X[6]) {
  rebvio::types::Matrix6f W = TooN::Zeros;
  rebvio::types::Vector6f x = TooN::Zeros;
  const bool ok = c->core->extRotVel(m->m, vec3(vel), W, x);
  for (int i = 0; i < 6; ++i) {
    X[i] = x[i];
    for (int j = 0; j < 6; ++j) Wx[i * 6 + j] = W(i, j);
  }
  return ok ? 1 : 0;
}
int ref_directed_match(ref_ctx*, ref_map* new_map, ref_map* old_map, const float vel[3], const float Rvel[9], const float Rback[9],
                       int* kf_matches, float max_radius) {
  int kf = 0;
  const int n = new_map->m->directedMatch(old_map->m, vec3(vel), mat3(Rvel), mat3(Rback), kf, max_radius);
  if (kf_matches) *kf_matches = kf;
  return n;
}
int ref_regularize(ref_map* m) { return m->m->regularize1Iter(); }
void ref_update_inverse_depth(ref_ctx* c, const float vel[3]) {
  rebvio::types::Vector3f v = vec3(vel);
  c->core->updateInverseDepth(v);
}

/* ---- inertial glue: the one function of it that is public and keeps no state between calls ---- */
void ref_gyro_bias_correction(ref_ctx* c, float X[6], float Wx[36], float Wb[9], const float Rg[9], const float Rb[9], float dgbias[3]) {
  rebvio::types::Vector6f x;
  rebvio::types::Matrix6f W;
  for (int i = 0; i < 6; ++i) {
    x[i] = X[i];
    for (int j = 0; j < 6; ++j) W(i, j) = Wx[i * 6 + j];
  }
  rebvio::types::Matrix3f B = mat3(Wb);
  const rebvio::types::Vector3f d = c->core->gyroBiasCorrection(x, W, B, mat3(Rg), mat3(Rb));
  for (int i = 0; i < 6; ++i) {
    X[i] = x[i];
    for (int j = 0; j < 6; ++j) Wx[i * 6 + j] = W(i, j);
  }
  for (int i = 0; i < 3; ++i) {
    dgbias[i] = d[i];
    for (int j = 0; j < 3; ++j) Wb[i * 3 + j] = B(i, j);
  }
}

/* ---- single-keyline forms ---- */
int ref_search_match(ref_ctx*, ref_map* searched, const orc_keyline* query, const float vel[3], const float Rvel[9],
                     const float Rback[9], float max_radius) {
  return searched->m->searchMatch(from_record(*query), vec3(vel), mat3(Rvel), mat3(Rback), max_radius);
}
float ref_calculate_fj(ref_ctx* c, ref_map* m, int f_inx, float* df_dx, float* df_dy, orc_keyline* keyline, float px, float py,
                       int* mnum, float* fi) {
  KeyLine k = from_record(*keyline);
  const float f = c->core->calculatefJ(m->m, f_inx, *df_dx, *df_dy, k, px, py, *mnum, *fi);
  std::memcpy(keyline, static_cast<const void*>(&k), sizeof(k));
  return f;
}
void ref_update_inverse_depth_arlu(ref_ctx* c, orc_keyline* keyline, const float vel[3]) {
  KeyLine k = from_record(*keyline);
  rebvio::types::Vector3f v = vec3(vel);
  c->core->updateInverseDepthARLU(k, v);
  std::memcpy(keyline, static_cast<const void*>(&k), sizeof(k));
}

}  // extern "C"
