// Edge tracking on gfx950: one thread per keyline, wavefront (64-lane) butterfly reductions, fixed-order
// block/grid reductions (deterministic), order-independent restatements of the reference's sequential
// "last writer wins" rules.
//
// Reference semantics (baumlin/rebvio): edge_map.cpp:39-259; core.cpp:39-261,417-456. Compiled with
// -ffp-contract=off; float/double promotion follows the reference expression by expression (see the
// oracle's header for the rules).
//
// Bound: HBM/L2 gather bandwidth (keyline SoA streams + distance-field / mask / matched-keyline gathers);
// no dense contraction exists on this path (largest product is 6x6), so MFMA does not apply.
#include "common.hpp"
#include "depth_prior.hpp"
#include "edge_chains.hpp"
#include "edge_segments.hpp"
#include "glue_dev.hpp"
#include "kf_cloud.hpp"
#include "stereo_prior.hpp"
#include "kf_handover.hpp"
#include "kf_pose.hpp"
#include "place.hpp"

#include <cstdlib>
#include <cstring>

namespace rh {

constexpr float kRhoMax = 20.0f;   // types/keyline.hpp:17
constexpr float kRhoMin = 1e-3f;   // types/keyline.hpp:18
constexpr float kRhoInit = 1.0f;   // types/keyline.hpp:19

struct Mat3 {
  float a[9];
};
struct Vec3 {
  float a[3];
};

__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// Wave total through the DPP data path (no LDS crossbar traffic, unlike __shfl_xor = ds_bpermute): Hillis-Steele steps
// inside each row of 16 lanes (row_shr 1,2,4,8, zero fill), then row_bcast15 into rows 1 and 3, row_bcast31 into rows
// 2 and 3. The total is valid in LANE 63 only; the tree is fixed, so results are reproducible.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add_f(float v) {
  const int moved = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xF, true);
  return v + __int_as_float(moved);
}
__device__ __forceinline__ float wave_total63_f(float v) {
  v = dpp_add_f<0x111, 0xF>(v);  // row_shr:1
  v = dpp_add_f<0x112, 0xF>(v);  // row_shr:2
  v = dpp_add_f<0x114, 0xF>(v);  // row_shr:4
  v = dpp_add_f<0x118, 0xF>(v);  // row_shr:8
  v = dpp_add_f<0x142, 0xA>(v);  // row_bcast:15 -> rows 1, 3
  v = dpp_add_f<0x143, 0xC>(v);  // row_bcast:31 -> rows 2, 3
  return v;
}
// The same tree for N independent values at once with fused v_add_f32_dpp (one VALU op per step and value instead of
// mov_dpp + add). Steps are emitted value-interleaved, so consecutive DPP reads of one register are N >= 8 instructions
// apart (gfx9 needs 2 wait states between a VALU write and a DPP read of the same VGPR; the leading s_nop covers the
// producer of the inputs). Disabled rows of the row_bcast steps keep their value, which is what the scan needs.
template <int N>
__device__ __forceinline__ void wave_total63_fN(float (&v)[N]) {
  static_assert(N >= 8, "dependent DPP ops must be at least 2 wait states apart");
  asm volatile("s_nop 1");
#define RH_DPP_STEP(ctrl)                                                             \
  _Pragma("unroll") for (int k = 0; k < N; ++k)                                       \
      asm volatile("v_add_f32_dpp %0, %0, %0 " ctrl : "+v"(v[k]));
  RH_DPP_STEP("row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0")
  RH_DPP_STEP("row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:0")
  RH_DPP_STEP("row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:0")
  RH_DPP_STEP("row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:0")
  RH_DPP_STEP("row_bcast:15 row_mask:0xa bank_mask:0xf")
  RH_DPP_STEP("row_bcast:31 row_mask:0xc bank_mask:0xf")
#undef RH_DPP_STEP
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Order-preserving float -> uint map (for atomicMax on rho).
__device__ __forceinline__ unsigned order_key(float f) {
  const unsigned b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// rotateKeylines for one keyline (edge_map.cpp:59-70). makeVector(float, float, 1.0) mixes float and double
// arguments: TooN's double overload is selected, so the matrix-vector product is accumulated in double and rounded
// to float once per component.
__device__ __forceinline__ void rotate_one(const Mat3& R, float fm, float2& pi, float2& rs, float2& g) {
  const double v0 = (double)(pi.x / fm), v1 = (double)(pi.y / fm);
  float q[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double s = 0.0;
    s += (double)R.a[i * 3 + 0] * v0;
    s += (double)R.a[i * 3 + 1] * v1;
    s += (double)R.a[i * 3 + 2] * 1.0;
    q[i] = (float)s;
  }
  if (fabsf(q[2]) > 0.0f) {
    pi.x = q[0] / q[2] * fm;
    pi.y = q[1] / q[2] * fm;
    rs.x /= q[2];
    rs.y /= q[2];
  }
  float gq[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    double s = 0.0;
    s += (double)R.a[i * 3 + 0] * (double)g.x;
    s += (double)R.a[i * 3 + 1] * (double)g.y;
    s += (double)R.a[i * 3 + 2] * 0.0;
    gq[i] = (float)s;
  }
  g = make_float2(gq[0], gq[1]);
}

// ---- EdgeMap::rotateKeylines (edge_map.cpp:58-71) [+ estimateQuantile histogram, :39-46] -------------------
// makeVector(float, float, 1.0) mixes float and double arguments: TooN's double overload is selected, so the
// matrix-vector product is accumulated in double and rounded to float once per component.
__global__ __launch_bounds__(256) void k_rotate(KParams p, MapDev m, Mat3 R, int* __restrict__ hist, int hist_bins,
                                                int zero_dm) {
  __shared__ int sh[128];
  const int idx = blockIdx.x * 256 + threadIdx.x;
  float2 pi = m.pos_img[idx];  // bound-free early loads
  float2 rs = m.rs[idx];
  float2 g = m.grad[idx];
  const int n = m.st->n;
  if (hist) {
    if (threadIdx.x < 128) sh[threadIdx.x] = 0;
    __syncthreads();
  }
  if (zero_dm && blockIdx.x == 0 && threadIdx.x == 0) {
    m.st->dm_matches = 0;
    m.st->dm_kf = 0;
    m.st->reg_count = 0;
    m.st->dm_queued = 0;
  }
  if (idx < n) {
    rotate_one(R, p.fm, pi, rs, g);
    m.pos_img[idx] = pi;
    m.rs[idx] = rs;
    m.grad[idx] = g;
    if (hist) {
      m.residual[idx] = 0.f;  // minimizeVel starts from residuals[] = {0} (core.cpp:158)
      int i = cvtt_f32(hist_bins * (rs.y - kRhoMin) / (kRhoMax - kRhoMin));
      i = (i > hist_bins - 1) ? (hist_bins - 1) : i;
      i = (i < 0) ? 0 : i;
      atomicAdd(&sh[i], 1);
    }
  }
  if (hist) {
    __syncthreads();
    if ((int)threadIdx.x < hist_bins && sh[threadIdx.x]) atomicAdd(&hist[threadIdx.x], sh[threadIdx.x]);
  }
}

// Histogram only (stand-alone EdgeMap::estimateQuantile).
__global__ __launch_bounds__(256) void k_sigma_hist(MapDev m, int* __restrict__ hist, int hist_bins) {
  __shared__ int sh[128];
  const int n = m.st->n;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (threadIdx.x < 128) sh[threadIdx.x] = 0;
  __syncthreads();
  if (idx < n) {
    int i = cvtt_f32(hist_bins * (m.rs[idx].y - kRhoMin) / (kRhoMax - kRhoMin));
    i = (i > hist_bins - 1) ? (hist_bins - 1) : i;
    i = (i < 0) ? 0 : i;
    atomicAdd(&sh[i], 1);
  }
  __syncthreads();
  if ((int)threadIdx.x < hist_bins && sh[threadIdx.x]) atomicAdd(&hist[threadIdx.x], sh[threadIdx.x]);
}

// Tail of estimateQuantile (edge_map.cpp:47-55): first bin whose running count (checked before adding the
// bin) exceeds percentile * size.
__device__ __forceinline__ float quantile_from_hist(const int* __restrict__ hist, int bins, float pct, int n) {
  float sigma_rho = 1e3f;
  int a = 0;
  for (int i = 0; i < bins; ++i) {
    if ((float)a > pct * (float)n) {
      sigma_rho = float(i) * (kRhoMax - kRhoMin) / float(bins) + kRhoMin;
      break;
    }
    a += hist[i];
  }
  return sigma_rho;
}

// The same on a whole wave (bins <= 128, two per lane): an exclusive prefix over the lanes' pairs replaces the up to `bins`
// dependent LDS reads of the loop above (1-2 us on a lone lane at the head of the persistent LM kernels). Integer counts:
// the same bin whatever the order. Every lane of ONE wave calls it; every lane returns the result.
__device__ __forceinline__ float quantile_from_hist_wave(const int* __restrict__ hist, int bins, float pct, int n, int lane) {
  const int h0 = (2 * lane < bins) ? hist[2 * lane] : 0;
  const int h1 = (2 * lane + 1 < bins) ? hist[2 * lane + 1] : 0;
  int incl = h0 + h1;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  const int before0 = incl - (h0 + h1), before1 = before0 + h0;  // running count when the loop reaches bin 2 lane / 2 lane + 1
  const float thr = pct * (float)n;
  const bool c0 = 2 * lane < bins && (float)before0 > thr;
  const bool c1 = 2 * lane + 1 < bins && (float)before1 > thr;
  const unsigned long long m = __ballot(c0 || c1);
  if (m == 0ull) return 1e3f;
  const int fl = __ffsll((long long)m) - 1;
  const int first = 2 * fl + (__shfl((int)c0, fl) ? 0 : 1);
  return float(first) * (kRhoMax - kRhoMin) / float(bins) + kRhoMin;
}

__global__ void k_quantile(MapDev m, const int* __restrict__ hist, int bins, float pct, float* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *out = quantile_from_hist(hist, bins, pct, m.st->n);
}

// ---- 3x3 helpers with the reference's operation order -------------------------------------------------------
// TooN::determinant for N = 3: Gaussian elimination with partial pivoting.
__device__ float det3_elim(const float* A_) {
  float A[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A[i][j] = A_[i * 3 + j];
  float det = 1;
  for (int i = 0; i < 3; ++i) {
    int argmax = i;
    float mx = fabsf(A[i][i]);
    for (int ii = i + 1; ii < 3; ++ii)
      if (fabsf(A[ii][i]) > mx) {
        mx = fabsf(A[ii][i]);
        argmax = ii;
      }
    const float pivot = A[argmax][i];
    if (argmax != i) {
      det *= -1;
      for (int ii = i; ii < 3; ++ii) {
        const float t = A[i][ii];
        A[i][ii] = A[argmax][ii];
        A[argmax][ii] = t;
      }
    }
    det *= A[i][i];
    if (det == 0) return 0;
    for (int u = i + 1; u < 3; ++u) {
      const float factor = A[u][i] / pivot;
      for (int uu = i; uu < 3; ++uu) A[u][uu] = A[u][uu] - factor * A[i][uu];
    }
  }
  return det;
}

// types::invert (types/definitions.hpp:40-53)
__device__ void invert3(const float* m, float* o) {
  o[0] = m[4] * m[8] - m[5] * m[7];
  o[1] = m[2] * m[7] - m[1] * m[8];
  o[2] = m[1] * m[5] - m[2] * m[4];
  o[3] = m[5] * m[6] - m[3] * m[8];
  o[4] = m[0] * m[8] - m[2] * m[6];
  o[5] = m[2] * m[3] - m[0] * m[5];
  o[6] = m[3] * m[7] - m[4] * m[6];
  o[7] = m[1] * m[6] - m[0] * m[7];
  o[8] = m[0] * m[4] - m[1] * m[3];
  const float d = det3_elim(m);
  for (int i = 0; i < 9; ++i) o[i] = o[i] / d;
}

__device__ __forceinline__ void sym6_to_9(const float* J, float* M) {
  M[0] = J[0]; M[1] = J[3]; M[2] = J[4];
  M[3] = J[3]; M[4] = J[1]; M[5] = J[5];
  M[6] = J[4]; M[7] = J[5]; M[8] = J[2];
}

// One Levenberg-Marquardt bookkeeping step of Core::minimizeVel (core.cpp:161-185), run redundantly and
// identically by thread 0 of every workgroup; `red` = fixed-order sum of the previous call's block records.
// call: index of the tryVel evaluation about to run (0..iterations); final: no further evaluation follows.
// The state lives in LDS and `red` may alias it as far as the compiler can tell, so working on it in place turns every
// field access into its own LDS round trip on a lone thread; the step therefore runs on register copies (same
// operations in the same order) and writes the state back once.
__device__ void lm_step_regs(LmState& s, const float (&red)[10], int call, bool final_only);
__device__ void lm_step(LmState& s_lds, const float* red_lds, int call, bool final_only) {
  LmState t = s_lds;
  float r[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) r[i] = red_lds[i];
  lm_step_regs(t, r, call, final_only);
  s_lds = t;
}
// core.cpp:180-183: the matrix JtJ + u * Identity as TooN forms it (every element gets its term), and the trial point from
// its inverse
__device__ __forceinline__ void lm_step_matrix(const LmState& s, float (&M)[9]) {
  sym6_to_9(s.JtJ, M);
  M[0] = M[0] + 1.0f * s.u;
  M[4] = M[4] + 1.0f * s.u;
  M[8] = M[8] + 1.0f * s.u;
  M[1] = M[1] + 0.0f * s.u; M[2] = M[2] + 0.0f * s.u; M[3] = M[3] + 0.0f * s.u;
  M[5] = M[5] + 0.0f * s.u; M[6] = M[6] + 0.0f * s.u; M[7] = M[7] + 0.0f * s.u;
}
__device__ __forceinline__ void lm_step_apply(LmState& s, const float (&inv)[9]) {
  const float neg[3] = {-s.JtF[0], -s.JtF[1], -s.JtF[2]};
  for (int i = 0; i < 3; ++i) {
    float acc = 0;
    for (int k = 0; k < 3; ++k) acc += inv[i * 3 + k] * neg[k];
    s.h[i] = acc;
  }
  for (int i = 0; i < 3; ++i) s.Vnew[i] = s.vel[i] + s.h[i];
}
// the accept / reject bookkeeping of one step (core.cpp:161-179)
__device__ __forceinline__ void lm_step_book(LmState& s, const float (&red)[10], int call) {
  if (call == 1) {
    s.F = red[0];
    for (int i = 0; i < 6; ++i) s.JtJ[i] = red[1 + i];
    for (int i = 0; i < 3; ++i) s.JtF[i] = red[7 + i];
    s.v = 2.0f;
    const float tau = 1e-3f;
    float mx = s.JtJ[0];
    for (int i = 1; i < 6; ++i)
      if (s.JtJ[i] > mx) mx = s.JtJ[i];
    s.u = tau * mx;
    s.accept_mask = 0;
  } else if (call >= 2) {
    const float Fnew = red[0];
    double den = 0.0;
    for (int i = 0; i < 3; ++i) den += (0.5 * (double)s.h[i]) * (double)(s.u * s.h[i] - s.JtF[i]);
    const float gain = (float)((double)(s.F - Fnew) / den);
    if (gain > 0.0f) {
      s.F = Fnew;
      for (int i = 0; i < 3; ++i) s.vel[i] = s.Vnew[i];
      for (int i = 0; i < 6; ++i) s.JtJ[i] = red[1 + i];
      for (int i = 0; i < 3; ++i) s.JtF[i] = red[7 + i];
      const double g = (double)gain;
      const double c = 1.0 - ((2.0 * g - 1.0) * (2.0 * g - 1.0) * (2.0 * g - 1.0));
      s.u = (float)((double)s.u * (0.33 > c ? 0.33 : c));
      s.v = 2.0f;
      s.accept_mask |= 1 << (call - 2);
    } else {
      s.u *= s.v;
      s.v = (float)((double)s.v * 2.0);
    }
  }
}
__device__ __forceinline__ void lm_step_regs(LmState& s, const float (&red)[10], int call, bool final_only) {
  lm_step_book(s, red, call);
  if (call >= 1 && !final_only) {
    float M[9], inv[9];
    lm_step_matrix(s, M);
    invert3(M, inv);
    lm_step_apply(s, inv);
  }
}

// The same step on a whole wave (every lane of wave 0 of a workgroup calls it, every workgroup alike): the bookkeeping on
// registers in every lane, the 3x3 inverse with one cofactor per lane (nine divisions side by side instead of in a row: the
// lone thread's step cost 0.9 us three times per launch), the new trial point from the inverse in LDS. Same operations per
// element, same bits. inv_lds: 9 floats of LDS.
__device__ __forceinline__ void lm_step_wave(LmState& s_lds, const float* red_lds, int call, bool final_only, float* inv_lds, int lane) {
  LmState t = s_lds;
  float r[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) r[i] = red_lds[i];
  lm_step_book(t, r, call);
  if (call >= 1 && !final_only) {
    float M[9];
    lm_step_matrix(t, M);
    const float d = glue_det3(M);
    float o;
    switch (lane) {
      case 0: o = M[4] * M[8] - M[5] * M[7]; break;
      case 1: o = M[2] * M[7] - M[1] * M[8]; break;
      case 2: o = M[1] * M[5] - M[2] * M[4]; break;
      case 3: o = M[5] * M[6] - M[3] * M[8]; break;
      case 4: o = M[0] * M[8] - M[2] * M[6]; break;
      case 5: o = M[2] * M[3] - M[0] * M[5]; break;
      case 6: o = M[3] * M[7] - M[4] * M[6]; break;
      case 7: o = M[1] * M[6] - M[0] * M[7]; break;
      default: o = M[0] * M[4] - M[1] * M[3]; break;
    }
    glue_wave_sync();  // (the previous step's inverse has been read by every lane)
    if (lane < 9) inv_lds[lane] = o / d;
    glue_wave_sync();
    float inv[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) inv[i] = inv_lds[i];
    lm_step_apply(t, inv);
  }
  if (lane == 0) s_lds = t;
}

// lm_step_wave for the step in front of a run of speculative evaluations (k_lm_chain_spec): besides the real state (q = 0) the
// wave forms, side by side in its four 16-lane rows, the states q = 1 .. 3 the NEXT steps start from if every one of them
// rejects - q rejections' (u, v) updates on the state the bookkeeping left (core.cpp:180-183: a rejection changes nothing
// else), then the trial point from that state's own inverse. One inverse's latency instead of two in a row; same operations
// per state as lm_step_book on a NaN score + lm_step_matrix + the inverse + lm_step_apply, same bits. stc[q] for q < nstates.
__device__ __forceinline__ void lm_step_wave_states(LmState& s_lds, const float* red_lds, int call, float (*inv_lds)[9], int lane,
                                                    LmState* stc, int nstates) {
  LmState t = s_lds;
  float r[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) r[i] = red_lds[i];
  lm_step_book(t, r, call);
  const int q = lane >> 4, e = lane & 15;
  for (int j = 0; j < q; ++j) {
    t.u *= t.v;
    t.v = (float)((double)t.v * 2.0);
  }
  float M[9];
  lm_step_matrix(t, M);
  const float d = glue_det3(M);
  float o;
  switch (e) {
    case 0: o = M[4] * M[8] - M[5] * M[7]; break;
    case 1: o = M[2] * M[7] - M[1] * M[8]; break;
    case 2: o = M[1] * M[5] - M[2] * M[4]; break;
    case 3: o = M[5] * M[6] - M[3] * M[8]; break;
    case 4: o = M[0] * M[8] - M[2] * M[6]; break;
    case 5: o = M[2] * M[3] - M[0] * M[5]; break;
    case 6: o = M[3] * M[7] - M[4] * M[6]; break;
    case 7: o = M[1] * M[6] - M[0] * M[7]; break;
    default: o = M[0] * M[4] - M[1] * M[3]; break;
  }
  glue_wave_sync();  // (the previous step's inverse has been read by every lane)
  if (e < 9) inv_lds[q][e] = o / d;
  glue_wave_sync();
  float inv[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) inv[i] = inv_lds[q][i];
  lm_step_apply(t, inv);
  if (e == 0 && q < nstates) stc[q] = t;
  if (lane == 0) s_lds = t;
}

// Shared prologue: fixed-order reduction of the previous tryVel call's block records + carry-in of the
// "last written fi" (oracle header, H3) for this workgroup. The records are staged in LDS by one coalesced
// pass of the whole workgroup (one memory round trip), then summed in block order from LDS.

// Stages the records of ALL launched workgroups (grid size is known without reading the keyline count, so these
// loads are in flight together with the first own-keyline loads); records beyond the live count are never summed.
__device__ void stage_prev_records(const float* __restrict__ part_prev, int grid_blocks, float* rec /*LDS*/) {
  const int total = min(grid_blocks, kMaxRecBlocks) * kPartStride;
  for (int i = threadIdx.x; i < total; i += blockDim.x) rec[i] = part_prev[i];
}

// Fixed-order sum of the staged records with 160 threads: sum k (0..9) lives in the 16-lane row k, lane j adds the
// records b = j, j+16, ... in ascending order, a DPP scan inside the row (row_shr 1,2,4,8) leaves the total in lane 15.
// `first_group` = index of this workgroup's first record group, `groups` = record groups it owns (carry_in[g] for each).
__device__ __forceinline__ void reduce_staged_records(const float* rec, int nblocks, float* red /*shared[16]*/, float* carry_in,
                                                      int first_group, int groups) {
  const int t = threadIdx.x;
  if (t < 160) {
    const int k = t >> 4, j = t & 15;
    float acc = 0.f;
    for (int b = j; b < nblocks; b += 16) acc += rec[b * kPartStride + k];
    acc = dpp_add_f<0x111, 0xF>(acc);
    acc = dpp_add_f<0x112, 0xF>(acc);
    acc = dpp_add_f<0x114, 0xF>(acc);
    acc = dpp_add_f<0x118, 0xF>(acc);
    if (j == 15) red[k] = acc;
  } else if (t >= 192 && t < 192 + groups) {
    const int g = t - 192;
    float cv = 0.f;
    for (int b = first_group + g - 1; b >= 0; --b)
      if (rec[b * kPartStride + 10] != 0.f) {
        cv = rec[b * kPartStride + 11];
        break;
      }
    carry_in[g] = fabsf(cv);
  }
}

// The ten sums of one staged record set by the 160 threads t0 .. t0 + 159 (same order as reduce_staged_records).
__device__ __forceinline__ void reduce_staged_sums(const float* rec, int nblocks, float* red /*shared[16]*/, int t0) {
  const int t = (int)threadIdx.x - t0;
  if (t >= 0 && t < 160) {
    const int k = t >> 4, j = t & 15;
    float acc = 0.f;
    for (int b = j; b < nblocks; b += 16) acc += rec[b * kPartStride + k];
    acc = dpp_add_f<0x111, 0xF>(acc);
    acc = dpp_add_f<0x112, 0xF>(acc);
    acc = dpp_add_f<0x114, 0xF>(acc);
    acc = dpp_add_f<0x118, 0xF>(acc);
    if (j == 15) red[k] = acc;
  }
}

// Per-keyline body of Core::tryVel / calculatefJ / testfk (core.cpp:39-148), shared by the per-call kernel and the
// persistent LM kernel.
struct TvIn {
  float gn;
  float2 rs, pi, g2;
  unsigned nmatches;
  // velocity-independent sub-expressions of calculatefJ, evaluated once per keyline instead of once per evaluation
  // (same operands, same operations -> same bits): 1/rho and 1/sigma in double, search_range / sigma
  double inv_rho_d, inv_sig_d;
  float range_over_sig;
};
__device__ __forceinline__ TvIn make_tvin(const KParams& p, float gn, float2 rs, float2 pi, float2 g2, unsigned nmatches) {
  TvIn k;
  k.gn = gn;
  k.rs = rs;
  k.pi = pi;
  k.g2 = g2;
  k.nmatches = nmatches;
  k.inv_rho_d = 1.0 / (double)rs.x;
  k.inv_sig_d = 1.0 / (double)rs.y;
  k.range_over_sig = p.search_range / rs.y;
  return k;
}
struct TvOut {
  float f, jx, jy, jz, fi, res_out;
  int mfwd;
  bool contrib, matched, need_carry, wrote_res;
};
// try_vel_eval in three steps, so that a caller with several trial velocities at hand (k_lm_chain_spec) can have the
// dependent gathers of all of them in flight together: (1) projection of the keyline under the trial velocity - no memory,
// nothing that depends on the residual; (2) the distance-field cell, then the geometry of the keyline it names; (3) the
// arithmetic, which is where the residual of the previous evaluation (the IRLS weight) comes in.
struct TvProj {
  float rho_p, p_x, p_y, p_xc, p_yc;
  int cell;  // y * cols + x, or -1 when there is no cell to look at (keyline skipped, or penalised before the lookup)
  bool skip, penalty1;
};
struct TvGeo {
  float2 g1, pn;
  float gnn;
  int id;  // -1: empty cell
};
__device__ __forceinline__ TvProj tv_project(const KParams& p, const TvIn& k, float vx, float vy, float vz, float srm, float thr,
                                             unsigned min_matches) {
  TvProj o{};
  o.cell = -1;
  o.skip = (thr > 0.0f && k.gn < thr) || (k.rs.y > srm) || (k.nmatches < min_matches);
  if (o.skip) return o;
  const float2 pi = k.pi;
  const float z_p = (float)(k.inv_rho_d + (double)vz);
  if (z_p <= 0.0f) {
    o.penalty1 = true;
  } else {
    o.rho_p = (float)(1.0 / (double)z_p);
    o.p_x = o.rho_p * (vx * p.fm - vz * pi.x) + pi.x;
    o.p_y = o.rho_p * (vy * p.fm - vz * pi.y) + pi.y;
    o.p_xc = o.p_x + p.cx;
    o.p_yc = o.p_y + p.cy;
    const int x = cvtt_f64((double)o.p_xc + 0.5);
    const int y = cvtt_f64((double)o.p_yc + 0.5);
    if (x < 1 || y < 1 || (unsigned)x >= (unsigned)p.cols - 1u || (unsigned)y >= (unsigned)p.rows - 1u)
      o.penalty1 = true;
    else
      o.cell = y * p.cols + x;
  }
  return o;
}
__device__ __forceinline__ unsigned tv_cell(const MapDev& nm, const TvProj& pj) { return pj.cell >= 0 ? nm.df[(size_t)pj.cell] : kDfEmpty; }
__device__ __forceinline__ TvGeo tv_geometry(const KParams& p, const MapDev& nm, unsigned key) {
  TvGeo g{};
  g.id = -1;
  if (key != kDfEmpty) {
    g.id = (int)((kDfSeqMask - (key & kDfSeqMask)) / (unsigned)p.df_nr);
    g.g1 = nm.grad[g.id];
    g.pn = nm.pos[g.id];  // issued with g1: one gather round trip
    g.gnn = nm.gnorm[g.id];
  }
  return g;
}
// (3a) what does not depend on the residual: the similarity test of the cell's keyline (testfk), fi and the gradient of f
struct TvMatch {
  float fi, df_dx, df_dy, f0;  // f0: f before the IRLS weight
  int mfwd;
  bool matched, need_carry;
};
__device__ __forceinline__ TvMatch tv_match(const KParams& p, const TvIn& k, const TvProj& pj, const TvGeo& ge) {
  TvMatch m{};
  m.mfwd = -1;
  if (pj.skip || pj.penalty1) return m;
  const float gn = k.gn;
  const float2 rs = k.rs, g2 = k.g2;
  if (ge.id >= 0) {
    const float2 g1 = ge.g1;
    const float norm_squared = gn * gn;
    const float dot_product = g1.x * g2.x + g1.y * g2.y;
    if (!(fabsf(dot_product - norm_squared) > p.match_treshold * norm_squared)) {
      const float dx = pj.p_xc - ge.pn.x;
      const float dy = pj.p_yc - ge.pn.y;
      const float gnx = g1.x / ge.gnn;
      const float gny = g1.y / ge.gnn;
      m.fi = (dx * gnx + dy * gny);
      m.df_dx = gnx / rs.y;
      m.df_dy = gny / rs.y;
      m.mfwd = ge.id;
      m.f0 = m.fi / rs.y;
      m.matched = true;
    }
  }
  if (!m.matched) {
    m.f0 = k.range_over_sig;
    m.need_carry = true;
  }
  return m;
}
// (3b) the IRLS weight from the previous evaluation's residual, and the weighted terms
__device__ __forceinline__ TvOut tv_weight(const KParams& p, const TvIn& k, const TvProj& pj, const TvMatch& m, float res_in, float cin) {
  float f = 0.f, jx = 0.f, jy = 0.f, jz = 0.f, res_out = 0.f;
  bool contrib = false, wrote_res = false;
  if (!pj.skip) {
    float res = res_in;
    if (res == kResidualCarry) res = cin;
    res_out = res;
    float weight = 1.0f;
    if (res > p.reweight_distance) weight = p.reweight_distance / res;
    contrib = true;
    if (pj.penalty1) {
      f = (float)((k.inv_sig_d * (double)p.search_range) * (double)weight);
    } else {
      f = m.f0;
      f *= weight;
      jx = pj.rho_p * p.fm * m.df_dx * weight;
      jy = pj.rho_p * p.fm * m.df_dy * weight;
      jz = -pj.rho_p * (pj.p_x * m.df_dx + pj.p_y * m.df_dy) * weight;
      if (m.matched) res_out = fabsf(m.fi);
    }
    wrote_res = !m.need_carry;
  }
  return TvOut{f, jx, jy, jz, m.fi, res_out, m.mfwd, contrib, m.matched, m.need_carry, wrote_res};
}
__device__ __forceinline__ TvOut tv_finish(const KParams& p, const TvIn& k, const TvProj& pj, const TvGeo& ge, float res_in, float cin) {
  return tv_weight(p, k, pj, tv_match(p, k, pj, ge), res_in, cin);
}
__device__ __forceinline__ TvOut try_vel_eval(const KParams& p, const MapDev& nm, const TvIn& k, float res_in, float cin, float vx,
                                              float vy, float vz, float srm, float thr, unsigned min_matches) {
  const TvProj pj = tv_project(p, k, vx, vy, vz, srm, thr, min_matches);
  const TvGeo ge = tv_geometry(p, nm, tv_cell(nm, pj));
  return tv_finish(p, k, pj, ge, res_in, cin);
}

// ---- Core::tryVel + calculatefJ + testfk (core.cpp:39-148) ---------------------------------------------------
// mode_lm = 0: evaluate at st_in->Vnew with st_in->sigma_rho_min (stand-alone tryVel).
// mode_lm = 1: call `call` of minimizeVel; prologue derives the LM state from the previous call's records.
// last: the evaluation whose side effects persist (core.cpp:166-185 never re-evaluates an accepted point):
//       matched keylines publish forwardMatch keys (edge_map.cpp:78-96) so that no extra pass is needed.
__global__ __launch_bounds__(256) void k_try_vel(KParams p, MapDev om, MapDev nm, int mode_lm, int call, int last,
                                                 const LmState* __restrict__ st_in, LmState* __restrict__ st_out,
                                                 const float* __restrict__ part_prev, float* __restrict__ part_out,
                                                 const int* __restrict__ hist, unsigned frame_count) {
  __shared__ LmState s;
  __shared__ float red[16];
  __shared__ float carry_in;
  __shared__ float wsum[4][10];
  __shared__ float wlast[4];
  __shared__ int whas[4];
  __shared__ float rec[kMaxRecBlocks * kPartStride];
  __shared__ int shist[128];

  // Own-keyline loads are issued before anything else (arrays are padded to the grid, so no bound is needed):
  // their latency overlaps the prologue instead of following it.
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const float gn = om.gnorm[idx];
  const float2 rs = om.rs[idx];
  const float2 pi = om.pos_img[idx];
  const float2 g2 = om.grad[idx];
  const unsigned nmatches = om.matches[idx];
  const float res_in = om.residual[idx];
  if (mode_lm && call >= 1) stage_prev_records(part_prev, gridDim.x, rec);
  const int n = om.st->n;
  const float thr = om.st->threshold;
  const int nblocks = (n + 255) / 256;
  if (mode_lm && call == 0 && threadIdx.x < 128) shist[threadIdx.x] = (threadIdx.x < (unsigned)p.quantile_num_bins) ? hist[threadIdx.x] : 0;
  if (threadIdx.x == 0) {
    carry_in = 0.f;
    s = *st_in;
  }
  __syncthreads();
  if (mode_lm && call >= 1) reduce_staged_records(rec, nblocks, red, &carry_in, (int)blockIdx.x, 1);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (mode_lm) {
      if (call == 0) {
        s.sigma_rho_min = quantile_from_hist(shist, p.quantile_num_bins, p.quantile_cutoff, n);
        for (int i = 0; i < 3; ++i) s.Vnew[i] = s.vel[i];
      } else {
        lm_step(s, red, call, false);
      }
    }
    if (blockIdx.x == 0) *st_out = s;
  }
  __syncthreads();
  if ((int)blockIdx.x >= nblocks && blockIdx.x != 0) return;

  const float vx = s.Vnew[0], vy = s.Vnew[1], vz = s.Vnew[2];
  const float srm = s.sigma_rho_min;
  const float cin = carry_in;
  const unsigned min_matches = min(p.min_match_threshold, frame_count);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;

  TvOut e{};
  e.mfwd = -1;
  if (idx < n) {
    const TvIn in = make_tvin(p, gn, rs, pi, g2, nmatches);
    e = try_vel_eval(p, nm, in, res_in, cin, vx, vy, vz, srm, thr, min_matches);
    if (e.wrote_res) om.residual[idx] = e.res_out;
    if (e.matched && last) {
      const unsigned long long key = ((unsigned long long)order_key(rs.x) << 32) | (unsigned)idx;
      atomicMax(&nm.fwd_key[e.mfwd], key);
    }
    om.match_fwd[idx] = e.mfwd;
  }
  const float f = e.f, jx = e.jx, jy = e.jy, jz = e.jz, fi = e.fi;
  const bool contrib = e.contrib, matched = e.matched, need_carry = e.need_carry;

  // carry-forward of the last written fi (index order) for calculatefJ's early-return paths
  const unsigned long long mm = __ballot(matched);
  const unsigned long long below = mm & ((1ull << lane) - 1ull);
  const int src = below ? (63 - __clzll((long long)below)) : 0;
  const float fi_prev = __shfl(fi, src);
  const int wl = mm ? (63 - __clzll((long long)mm)) : 0;
  const float fi_wlast = __shfl(fi, wl);
  if (lane == 0) {
    whas[wid] = mm ? 1 : 0;
    wlast[wid] = fi_wlast;
  }

  const float sc = contrib ? f * f : 0.f;
  float v[10] = {sc, jx * jx, jy * jy, jz * jz, jx * jy, jx * jz, jy * jz, jx * f, jy * f, jz * f};
  wave_total63_fN(v);
  if (lane == 63) {
#pragma unroll
    for (int k = 0; k < 10; ++k) wsum[wid][k] = v[k];
  }
  __syncthreads();
  if (need_carry) {
    float r;
    if (below) {
      r = fabsf(fi_prev);
    } else {
      r = kResidualCarry;
      for (int w = wid - 1; w >= 0; --w)
        if (whas[w]) {
          r = fabsf(wlast[w]);
          break;
        }
    }
    om.residual[idx] = r;
  }
  if (threadIdx.x < 10) {
    float acc = 0.f;
    for (int w = 0; w < 4; ++w) acc += wsum[w][threadIdx.x];
    part_out[blockIdx.x * kPartStride + threadIdx.x] = acc;
  } else if (threadIdx.x == 10) {
    float hv = 0.f, lv = 0.f;
    for (int w = 3; w >= 0; --w)
      if (whas[w]) {
        hv = 1.f;
        lv = wlast[w];
        break;
      }
    part_out[blockIdx.x * kPartStride + 10] = hv;
    part_out[blockIdx.x * kPartStride + 11] = lv;
  }
}

// Final accept/reject of minimizeVel for the stand-alone entry (the fused path does this in k_ext_rot_vel).
__global__ __launch_bounds__(256) void k_lm_final(MapDev om, int calls, const LmState* __restrict__ st_in,
                                                 LmState* __restrict__ st_out, const float* __restrict__ part_prev) {
  __shared__ float red[16];
  __shared__ float carry_in;
  __shared__ float rec[kMaxRecBlocks * kPartStride];
  // only the live groups: the launch has one workgroup, and the records of one evaluation are as many as the context's keyline
  // budget has groups - staging kMaxRecBlocks of them read past the end of the buffer for budgets under 16 k keylines
  const int nb = (om.st->n + 255) / 256;
  stage_prev_records(part_prev, nb, rec);
  __syncthreads();
  reduce_staged_records(rec, nb, red, &carry_in, 0, 1);
  __syncthreads();
  if (threadIdx.x == 0) {
    LmState s = *st_in;
    lm_step(s, red, calls, true);
    *st_out = s;
  }
}

// Stand-alone forwardMatch keys from match_id_forward (for the stepwise API; the fused path publishes the
// keys from the last tryVel evaluation).
__global__ __launch_bounds__(256) void k_forward_keys(MapDev om, MapDev nm) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= om.st->n) return;
  const int j = om.match_fwd[idx];
  if (j < 0) return;
  const unsigned long long key = ((unsigned long long)order_key(om.rs[idx].x) << 32) | (unsigned)idx;
  atomicMax(&nm.fwd_key[j], key);
}

// Per-keyline body of forwardMatch's gather (edge_map.cpp:78-96) and of extRotVel's row (core.cpp:198-245), shared by
// the per-call kernel and the persistent LM kernel.
struct XrvIn {
  unsigned long long key;
  int mid;
  float2 rs, mpi, g;
  float gn;
  float2 q;
};
// The forwardMatch gather of one keyline of the new map as loads only (what the old keyline named by `key` hands over):
// a caller that knows the keys early (k_lm_chain_spec) has these in flight while it still decides where the velocity ends up.
struct XrvFwd {
  float2 rs, mpi, mgrad;
  float mgnorm;
  unsigned matches;
  int kf, o;  // o < 0: nobody matched into this keyline
};
__device__ __forceinline__ XrvFwd xrv_gather(const MapDev& om, unsigned long long key) {
  XrvFwd f{};
  f.o = -1;
  if (key != 0ull) {
    const int o = (int)(unsigned)(key & 0xFFFFFFFFull);
    f.o = o;
    f.rs = om.rs[o];
    f.mpi = om.pos_img[o];
    f.matches = om.matches[o];
    f.mgrad = om.grad[o];
    f.mgnorm = om.gnorm[o];
    f.kf = om.match_kf[o];
  }
  return f;
}
__device__ __forceinline__ void xrv_apply(const KParams& p, MapDev& nm, int idx, int do_forward, const XrvFwd& f, XrvIn k, float vx,
                                          float vy, float vz, float row[6], float* Y_out, int* cnt_out) {
  float2 rs = k.rs, mpi = k.mpi;
  int mid = k.mid;
  if (do_forward) {
    // edge_map.cpp:83: a target that is already matched and holds a larger rho than the winning writer keeps what it has (a
    // map fresh from detection has match_id = -1 everywhere)
    if (f.o >= 0 && !(k.mid >= 0 && k.rs.x > f.rs.x)) {
      const int o = f.o;
      rs = f.rs;
      mpi = f.mpi;
      mid = o;
      nm.rs[idx] = rs;
      nm.matches[idx] = f.matches + 1u;
      nm.match_id[idx] = o;
      nm.mpos_img[idx] = mpi;
      nm.mgrad[idx] = f.mgrad;
      nm.mgnorm[idx] = f.mgnorm;
      nm.match_kf[idx] = f.kf;
    }
  }
  if (mid >= 0) {
    const float u_x = k.g.x / k.gn;
    const float u_y = k.g.y / k.gn;
    const float rho_t = (float)(1.0 / (1.0 / (double)rs.x + (double)vz));
    const float qt_x = mpi.x + rho_t * (vx * p.fm - vz * mpi.x);
    const float qt_y = mpi.y + rho_t * (vy * p.fm - vz * mpi.y);
    const float q_x = k.q.x, q_y = k.q.y;
    row[0] = u_x * rho_t * p.fm;
    row[1] = u_y * rho_t * p.fm;
    row[2] = u_x * (-rho_t * q_x) + u_y * (-rho_t * q_y);
    row[3] = -u_x * q_x * q_y / p.fm - u_y * (p.fm + q_y * q_y / p.fm);
    row[4] = u_y * q_x * q_y / p.fm + u_x * (p.fm + q_x * q_x / p.fm);
    row[5] = -u_x * q_y + u_y * q_x;
    float Y = u_x * (q_x - qt_x) + u_y * (q_y - qt_y);
    const float dqvel = u_x * (vx * p.fm - vz * mpi.x) + u_y * (vy * p.fm - vz * mpi.y);
    const float s_y = sqrtf(rs.y * rs.y * dqvel * dqvel + p.pixel_uncertainty * p.pixel_uncertainty);
    float weight = 1.0f;
    if (fabsf(Y) > p.reweight_distance) weight = fabsf(Y) / p.reweight_distance;
    const float dv = s_y * weight;
#pragma unroll
    for (int i = 0; i < 6; ++i) row[i] /= dv;
    Y /= dv;
    *Y_out = Y;
    *cnt_out = 1;
  }
}
__device__ __forceinline__ void xrv_eval(const KParams& p, const MapDev& om, MapDev& nm, int idx, int do_forward, XrvIn k, float vx,
                                         float vy, float vz, float row[6], float* Y_out, int* cnt_out) {
  const XrvFwd f = xrv_gather(om, do_forward ? k.key : 0ull);
  xrv_apply(p, nm, idx, do_forward, f, k, vx, vy, vz, row, Y_out, cnt_out);
}

// Sequence stamp of one extRotVel block record (kXrvStride floats: 27 sums, the match count, two spare words, a checksum, the stamp),
// called by the 32 lanes that own the record's words right after they stored them (`bits` = what lane k stored, 0 for k >= 28): the
// wave waits for its stores (vmcnt(0)), lane 30 stores the XOR of the record's words ^ seq, lane 31 the stamp. A host that polls
// the record accepts it when stamp AND checksum fit: the record is 128 bytes = two 64-byte writes on the way to host memory, and
// writes to host memory may arrive out of order.
__device__ __forceinline__ void xrv_record_stamp(float* rec, int k, unsigned seq, unsigned bits) {
  unsigned x = bits;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) x ^= (unsigned)__shfl_xor((int)x, o);  // (stays inside the 32-lane half that owns the record)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) (see stamp_drain)
  if (k == kXrvStride - 2) __hip_atomic_store(reinterpret_cast<unsigned*>(rec + k), x ^ seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (k == kXrvStride - 1) __hip_atomic_store(reinterpret_cast<unsigned*>(rec + k), seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- EdgeMap::forwardMatch gather (edge_map.cpp:78-96) + Core::extRotVel sums (core.cpp:198-245) -------------
// Sequential rule "overwrite unless the target already holds a larger rho" == the writer with the largest
// rho wins, ties -> largest index: exactly the atomicMax key; a target that came in matched is one more contender, which
// keeps its fields unless that writer's rho reaches its own (xrv_apply). One thread per keyline of the NEW map.
// Per-thread outer product of the 6-vector row (Phi is never materialised): 21 + 6 sums + match count.
__global__ __launch_bounds__(256) void k_ext_rot_vel(KParams p, MapDev om, MapDev nm, int do_forward, int do_lm_final,
                                                     int calls, const LmState* __restrict__ st_in,
                                                     LmState* __restrict__ st_out, const float* __restrict__ part_prev,
                                                     float* __restrict__ xrv_part, Vec3 vel_manual,
                                                     PairSlot* __restrict__ slot, int* __restrict__ hist_to_zero, unsigned seq) {
  unsigned slot_sum = 0u;  // XOR of the words this thread stored into the result slot (PairSlot::sum)
  __shared__ LmState s;
  __shared__ float red[16];
  __shared__ float carry_in;
  __shared__ float wsum[4][28];
  __shared__ float rec[kMaxRecBlocks * kPartStride];
  // early, bound-free loads of this thread's own keyline (arrays are padded to the grid)
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const unsigned long long key = nm.fwd_key[idx];
  int mid = nm.match_id[idx];
  float2 rs = nm.rs[idx];
  float2 mpi = nm.mpos_img[idx];
  const float2 g = nm.grad[idx];
  const float gn = nm.gnorm[idx];
  const float2 q = nm.pos_img[idx];
  const int n = nm.st->n;
  if (do_lm_final) {
    stage_prev_records(part_prev, gridDim.x, rec);
    const int nb_old = (om.st->n + 255) / 256;
    if (threadIdx.x == 0) s = *st_in;
    __syncthreads();
    reduce_staged_records(rec, nb_old, red, &carry_in, (int)blockIdx.x, 1);
    __syncthreads();
    if (threadIdx.x == 0) {
      lm_step(s, red, calls, true);
      if (blockIdx.x == 0) {
        *st_out = s;
        if (slot) slot_sum = slot_fill(slot, s, nm.st, om.st);  // zero-copy: the host reads these once the stamps say so
      }
    }
    __syncthreads();
  }
  // every tryVel call of this pair has consumed the sigma_rho histogram: clear it for the next pair
  if (hist_to_zero && blockIdx.x == 0 && threadIdx.x < 128) hist_to_zero[threadIdx.x] = 0;
  const float vx = do_lm_final ? s.vel[0] : vel_manual.a[0];
  const float vy = do_lm_final ? s.vel[1] : vel_manual.a[1];
  const float vz = do_lm_final ? s.vel[2] : vel_manual.a[2];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;

  float row[6] = {0, 0, 0, 0, 0, 0};
  float Y = 0.f;
  int cnt = 0;
  if (idx < n) {
    XrvIn k{key, mid, rs, mpi, g, gn, q};
    xrv_eval(p, om, nm, idx, do_forward, k, vx, vy, vz, row, &Y, &cnt);
  }
  float v[28];
  {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) v[k++] = row[i] * row[j];
#pragma unroll
    for (int i = 0; i < 6; ++i) v[21 + i] = row[i] * Y;
    v[27] = (float)cnt;
  }
  wave_total63_fN(v);
  if (lane == 63) {
#pragma unroll
    for (int k = 0; k < 28; ++k) wsum[wid][k] = v[k];
  }
  __syncthreads();
  unsigned stored = 0u;
  if (threadIdx.x < 28) {
    float acc = 0.f;
    for (int w = 0; w < 4; ++w) acc += wsum[w][threadIdx.x];
    xrv_part[blockIdx.x * kXrvStride + threadIdx.x] = acc;
    stored = __float_as_uint(acc);
  }
  if (threadIdx.x < 32) xrv_record_stamp(xrv_part + (size_t)blockIdx.x * kXrvStride, (int)threadIdx.x, seq, stored);
  if (slot && blockIdx.x == 0 && threadIdx.x == 0) {  // (block 0's own stores: lm, map states, its record)
    slot->sum = slot_sum ^ seq;
    stamp_drain(&slot->seq, seq);
  }
}

// ---- persistent minimizeVel + forwardMatch + extRotVel (core.cpp:150-245, edge_map.cpp:78-96) --------------------
// One launch instead of iterations+2: every workgroup keeps its keylines in registers across the LM evaluations and the
// workgroups exchange their block records after each evaluation. Records stay per 256 keylines ("record groups") and
// are summed in the same fixed order as in the per-call kernels, so both paths produce identical bits.
// The exchange is the grid barrier: every record word is published as one 64-bit agent-scope store {tag, float bits},
// tag = tag_base + evaluation index + 1 (unique over the life of the context, never 0), into the parity slot of the
// evaluation; every workgroup polls the words of all live record groups until they carry the tag - one memory round
// trip per evaluation, no contended counter, cost independent of the number of workgroups. A consumer that has seen
// evaluation c of every group knows every workgroup has finished reading evaluation c-1, so two parity slots suffice.
// A poll that lasts longer than kXchSpinLimit iterations (~0.2 s) raises *err and goes on: the grid always drains.
constexpr unsigned kXchSpinLimit = 1u << 18;

// The hand-off of the forwardMatch side effects (fwd_key atomics) to the other workgroups of the launch:
//   producer: every wave that issued them runs vm_drain() - a workgroup-scope release fence (compiler ordering: nothing it
//             issued before may sink below; on gfx942 / gfx950 outside tgsplit mode it emits no cache operation) followed by
//             "s_waitcnt vmcnt(0)": the atomics are performed at the device's coherence point (agent scope) and ACKNOWLEDGED
//             before the workgroup barrier behind which the record words that announce them go out (xch_publish);
//   consumer: polls the words (xch_wait), then xch_acquire() - a workgroup-scope acquire fence (compiler ordering: nothing
//             behind it may be hoisted above the polls) - then reads the keys with agent-scope ATOMIC loads, which are served
//             by the same coherence point and are issued in program order behind the poll that saw the tag.
// Everything that crosses workgroups inside these kernels is an agent-scope atomic word; no plain store is ever read by
// another workgroup of the same launch (match_fwd etc. are consumed by later kernels). What is deliberately NOT used is an
// agent-scope fence: the release form writes the XCD's L2 back (15 us per pair), the acquire form
// (buffer_inv sc1) invalidates the XCD's non-coherently cached L2 lines for every kernel running beside this one - measured
// -4 % frames/s on one stream and -5 % with 8 lanes (13.04 k -> 12.5 k, 39.1 k -> 37.2 k, same box, alternating runs), against
// no measurable cost for the workgroup-scope pair. The s_waitcnt immediate is the gfx9 encoding, where vmcnt counts loads,
// stores AND atomics of the wave; targets with a separate store counter (gfx10+) need another one, hence the guard.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx942__) && !defined(__gfx950__)
#error "track.hip: vm_drain() encodes s_waitcnt for gfx942 / gfx950 only"
#endif
__device__ __forceinline__ void vm_drain() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0); expcnt / lgkmcnt untouched
}
__device__ __forceinline__ void fwd_key_max(unsigned long long* w, unsigned long long key) {
  (void)__hip_atomic_fetch_max(w, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void xch_acquire() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); }

__device__ __forceinline__ void xch_publish(unsigned long long* w, unsigned tag, float v) {
  __hip_atomic_store(w, ((unsigned long long)tag << 32) | (unsigned long long)__float_as_uint(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}
// g_poll_sleep_long (set per launch through a kernel argument copied to a register): batched launches run several lanes'
// workgroups at once and every polling thread is an L2 request per poll - they back off longer between polls.
__device__ __forceinline__ float xch_wait(const unsigned long long* w, unsigned tag, int* err, int slow = 0) {
  unsigned spins = 0;
  unsigned long long v = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while ((unsigned)(v >> 32) != tag) {
    if (slow)
      __builtin_amdgcn_s_sleep(12);
    else
      __builtin_amdgcn_s_sleep(1);
    if (++spins > kXchSpinLimit) {
      // err[0] = flag, err[1..7] = diagnostics of the first waiter that gave up (host-visible pinned memory)
      if (__hip_atomic_exchange(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0) {
        err[1] = (int)blockIdx.x;
        err[2] = (int)threadIdx.x;
        err[3] = (int)tag;
        err[4] = (int)(unsigned)(v >> 32);
        err[5] = (int)(unsigned)v;
        err[6] = (int)gridDim.x;
        err[7] = (int)(reinterpret_cast<uintptr_t>(w) & 0x7FFFFFFFu);
      }
      break;
    }
    v = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return __uint_as_float((unsigned)v);
}

// Up to N words per thread polled TOGETHER: every round re-loads the words still missing in one batch (one memory round trip
// per round whatever their number), until all carry their tags. Waiting for them one after the other costs a round trip per
// word once the first has arrived; loading all once and then waiting one by one (tried) adds a round trip in the usual case
// that nothing is out yet. ok[j] false = no word for this thread in slot j. Same bound and diagnostics as xch_wait.
template <int N>
__device__ __forceinline__ void xch_wait_many(const unsigned long long* const (&w)[N], const unsigned (&tag)[N], const bool (&ok)[N],
                                              float (&out)[N], int* err, int slow) {
  bool have[N];
  bool all = true;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    have[j] = !ok[j];
    out[j] = 0.f;
    all = all && have[j];
  }
  unsigned spins = 0;
  while (!all) {
    unsigned long long v[N];
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (!have[j]) v[j] = __hip_atomic_load(w[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    all = true;
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (!have[j]) {
        if ((unsigned)(v[j] >> 32) == tag[j]) {
          have[j] = true;
          out[j] = __uint_as_float((unsigned)v[j]);
        } else {
          all = false;
        }
      }
    if (all) break;
    if (slow)
      __builtin_amdgcn_s_sleep(12);
    else
      __builtin_amdgcn_s_sleep(1);
    if (++spins > kXchSpinLimit) {
      if (__hip_atomic_exchange(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0) {
        err[1] = (int)blockIdx.x;
        err[2] = (int)threadIdx.x;
        err[3] = (int)tag[0];
        err[4] = 0;
        err[5] = 0;
        err[6] = (int)gridDim.x;
        err[7] = -3;
      }
      break;
    }
  }
}

// Wait for the records every live group published for evaluation `tag`, stage them in LDS and reduce them.
template <int kChainThreads>
__device__ __forceinline__ void chain_collect_records(const unsigned long long* __restrict__ slot_words, unsigned tag, int nblocks,
                                                      float* rec, float* red, float* carry_in, int* err, int slow = 0) {
  constexpr int kChainGroups = kChainThreads / 256;
  const int total = min(nblocks, kMaxRecBlocks) * kPartStride;
  for (int i = threadIdx.x; i < total; i += kChainThreads)
    if ((i & (kPartStride - 1)) < 12) rec[i] = xch_wait(slot_words + i, tag, err, slow);
  __syncthreads();
  reduce_staged_records(rec, nblocks, red, carry_in, (int)blockIdx.x * kChainGroups, kChainGroups);
  __syncthreads();
}

__device__ __forceinline__ GlueArgs lane_glue_args(const LaneStatic& L, const LaneDyn& d, int calls, const GlueParams& gp,
                                                   const float (&R_next)[9]) {
  GlueArgs ga;
  ga.lm = gptr(L.lm) + calls + 1;
  ga.xrv = gptr(L.xrv_part);
  ga.st_in = gptr(L.gstate) + (d.gpar & 1);
  ga.st_out = gptr(L.gstate) + ((d.gpar & 1) ^ 1);
  ga.rec = gptr(L.rec[d.slot]);
  ga.gd_copy = gptr(L.glue_dev) + d.slot;
  ga.stage = gptr(L.glue_stage) + d.slot;
  ga.seq = d.seq;
  // (only the scalars: a batch forms the gyroBiasCorrection matrices on the device - has_pre = 0 as a constant lets the compiler
  // drop the by-value matrices; copying them put the whole struct into scratch memory, 280 bytes per lane of every workgroup)
  ga.gp.frame_dt = gp.frame_dt;
  ga.gp.gyro_std_dev = gp.gyro_std_dev;
  ga.gp.gyro_bias_std_dev = gp.gyro_bias_std_dev;
  ga.gp.has_pre = 0;
  // the lane's own gyro rotation for its next pair (a batch always knows it: its flush ends every lane's stream)
  ga.gp.has_next = 1;
#pragma unroll
  for (int i = 0; i < 9; ++i) ga.gp.R_next[i] = R_next[i];
  return ga;
}

// Tail of the persistent LM kernels when the pair's glue runs on the device (ga.lm != null): every workgroup publishes the
// extRotVel sums of its record groups as tagged words (the exchange of the LM records, one more round), workgroup 0 waits
// for the groups that hold live keylines of the new map, sums them in group order in double (hm::sum_xrv) and runs the
// glue (glue_dev.hpp). The other workgroups leave right after publishing. stage: LDS, stage_groups * 32 floats.
template <int kChainThreads>
__device__ __forceinline__ void lm_tail_glue(const GlueArgs& ga, unsigned long long* __restrict__ xch_xrv, unsigned tag, int n_new,
                                             float* stage, int stage_groups, GlueLds& gw, const LmState& s, int* err, int slow,
                                             unsigned long long* stamps) {
  if (blockIdx.x != 0) return;
  const int tid = threadIdx.x;
  const int nb = (n_new + 255) / 256;
  double acc = 0.0;
  for (int b0 = 0; b0 < nb; b0 += stage_groups) {
    const int cnt = min(stage_groups, nb - b0);
    // a thread's words are polled TOGETHER (one memory round trip per round whatever their number, see xch_wait_many)
    for (int i0 = 0; i0 < cnt * kXrvStride; i0 += kChainThreads * 4) {
      const unsigned long long* w4[4];
      unsigned t4[4];
      bool ok4[4];
      float o4[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = i0 + j * kChainThreads + tid;
        ok4[j] = i < cnt * kXrvStride && (i & (kXrvStride - 1)) < 27;
        w4[j] = xch_xrv + (size_t)b0 * kXrvStride + min(i, cnt * kXrvStride - 1);
        t4[j] = tag;
      }
      xch_wait_many<4>(w4, t4, ok4, o4, err, slow);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (ok4[j]) stage[i0 + j * kChainThreads + tid] = o4[j];
    }
    __syncthreads();
    if (tid < 27)
      for (int b = 0; b < cnt; ++b) acc += (double)stage[b * kXrvStride + tid];
    __syncthreads();
  }
  if (tid < 21) {  // upper triangle in row-major order -> both halves of the symmetric matrix
    int i = 0, base = 0;
    while (tid >= base + (6 - i)) {
      base += 6 - i;
      ++i;
    }
    const int j = i + (tid - base);
    gw.W[i * 6 + j] = (float)acc;
    gw.W[j * 6 + i] = (float)acc;
  } else if (tid < 27) {
    gw.JtF[tid - 21] = (float)acc;
  }
  __syncthreads();
  if (stamps && tid == 0) stamps[16] = __builtin_amdgcn_s_memrealtime();
  glue_workgroup(gw, s, ga, stamps);
}

template <int kChainThreads>
__device__ __forceinline__ void lm_chain_body(KParams p, MapDev om, MapDev nm, int calls, int do_ext,
                                                            const LmState* __restrict__ st_in, LmState* __restrict__ st_out,
                                                            unsigned long long* __restrict__ xch, unsigned tag_base,
                                                            int* __restrict__ bar_err, const int* __restrict__ hist,
                                                            unsigned frame_count, float* __restrict__ xrv_part,
                                                            PairSlot* __restrict__ slot, int* __restrict__ hist_to_zero,
                                                            unsigned long long* __restrict__ stamps, int slow_poll, const GlueArgs ga) {
  unsigned slot_sum = 0u;  // XOR of the words thread 0 of workgroup 0 stored into the result slot (PairSlot::sum)
  constexpr int kChainGroups = kChainThreads / 256;
  __shared__ GlueLds gw;
  __shared__ float lm_inv[9];
  // optional phase stamps of workgroup 0 (REBVIO_HIP_LM_STAMPS diagnostic): 100 MHz constant clock
#define RH_STAMP(i) \
  do { if (stamps && blockIdx.x == 0 && threadIdx.x == 0) stamps[(i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
  __shared__ LmState s;
  __shared__ float red[16];
  __shared__ float carry_in[kChainGroups];
  __shared__ float wsum[kChainThreads / 64][28];
  __shared__ float wlast[kChainThreads / 64];
  __shared__ int whas[kChainThreads / 64];
  __shared__ float rec[kMaxRecBlocks * kPartStride];
  __shared__ int shist[128];

  const int tid = threadIdx.x;
  const int idx = blockIdx.x * kChainThreads + tid;
  const int lane = tid & 63, wid = tid >> 6, grp = tid >> 8, wig = wid & 3;
  const int nrec_launched = gridDim.x * kChainGroups;
  // own keyline of the old map (tryVel) and of the new map (extRotVel): loaded once, bound-free (arrays are padded)
  const TvIn in = make_tvin(p, om.gnorm[idx], om.rs[idx], om.pos_img[idx], om.grad[idx], om.matches[idx]);
  float res = om.residual[idx];
  XrvIn xk{};
  if (do_ext) {
    xk.mid = nm.match_id[idx];
    xk.rs = nm.rs[idx];
    xk.mpi = nm.mpos_img[idx];
    xk.g = nm.grad[idx];
    xk.gn = nm.gnorm[idx];
    xk.q = nm.pos_img[idx];
  }
  const int n = om.st->n;
  const float thr = om.st->threshold;
  const int n_new = nm.st->n;
  const int nblocks = (n + 255) / 256;
  if (tid < 128) shist[tid] = (tid < p.quantile_num_bins) ? hist[tid] : 0;
  if (tid == 0) s = *st_in;
  if (tid < kChainGroups) carry_in[tid] = 0.f;
  __syncthreads();
  if (tid < 64) {
    const float q = quantile_from_hist_wave(shist, p.quantile_num_bins, p.quantile_cutoff, n, tid);
    if (tid == 0) {
      s.sigma_rho_min = q;
      for (int i = 0; i < 3; ++i) s.Vnew[i] = s.vel[i];
    }
  }
  __syncthreads();
  const unsigned min_matches = min(p.min_match_threshold, frame_count);
  RH_STAMP(0);
  // A workgroup none of whose record groups holds a live keyline of the OLD map takes no part in the LM exchange: the
  // others do not wait for its records, so it could fall arbitrarily far behind them and find the parity slots already
  // rewritten. It only needs the final velocity for the extRotVel rows of its NEW-map keylines, which workgroup 0
  // broadcasts under the launch's last tag. (Workgroup 0 always runs the loop, also for an empty old map.)
  const bool lm_live = blockIdx.x == 0 || (int)blockIdx.x * kChainGroups < nblocks;
  unsigned long long* xch_final = xch + (size_t)2 * nrec_launched * kPartStride;
  const unsigned tag_final = tag_base + (unsigned)calls + 1u;

  for (int call = 0; lm_live && call < calls; ++call) {
    RH_STAMP(1 + call * 6 + 0);
    if (call >= 1) {
      chain_collect_records<kChainThreads>(xch + (size_t)((call - 1) & 1) * nrec_launched * kPartStride, tag_base + (unsigned)call, nblocks,
                                           rec, red, carry_in, bar_err, slow_poll);
      RH_STAMP(1 + call * 6 + 1);
      if (tid < 64) lm_step_wave(s, red, call, false, lm_inv, tid);
      __syncthreads();
    } else {
      RH_STAMP(1 + call * 6 + 1);
    }
    RH_STAMP(1 + call * 6 + 2);
    const float vx = s.Vnew[0], vy = s.Vnew[1], vz = s.Vnew[2];
    const float srm = s.sigma_rho_min;
    const float cin = carry_in[grp];
    const bool last = call == calls - 1;
    TvOut e{};
    e.mfwd = -1;
    if (idx < n) {
      e = try_vel_eval(p, nm, in, res, cin, vx, vy, vz, srm, thr, min_matches);
      if (e.wrote_res) res = e.res_out;
      if (last) {
        if (e.matched) {
          const unsigned long long key = ((unsigned long long)order_key(in.rs.x) << 32) | (unsigned)idx;
          fwd_key_max(&nm.fwd_key[e.mfwd], key);
        }
        om.match_fwd[idx] = e.mfwd;
      }
    }
    // last evaluation: this wave's forwardMatch atomics are acknowledged before the workgroup publishes its records (see
    // k_lm_chain_spec; a release fence on the publishing threads would order only their own operations)
    if (last) vm_drain();
    RH_STAMP(1 + call * 6 + 3);
    // carry-forward of the last written fi in index order (see k_try_vel)
    const unsigned long long mm = __ballot(e.matched);
    const unsigned long long below = mm & ((1ull << lane) - 1ull);
    const int src = below ? (63 - __clzll((long long)below)) : 0;
    const float fi_prev = __shfl(e.fi, src);
    const int wl = mm ? (63 - __clzll((long long)mm)) : 0;
    const float fi_wlast = __shfl(e.fi, wl);
    if (lane == 0) {
      whas[wid] = mm ? 1 : 0;
      wlast[wid] = fi_wlast;
    }
    const float sc = e.contrib ? e.f * e.f : 0.f;
    float v[10] = {sc, e.jx * e.jx, e.jy * e.jy, e.jz * e.jz, e.jx * e.jy, e.jx * e.jz, e.jy * e.jz, e.jx * e.f, e.jy * e.f, e.jz * e.f};
    wave_total63_fN(v);
    if (lane == 63) {
#pragma unroll
      for (int k = 0; k < 10; ++k) wsum[wid][k] = v[k];
    }
    __syncthreads();
    RH_STAMP(1 + call * 6 + 4);
    if (e.need_carry) {
      float r;
      if (below) {
        r = fabsf(fi_prev);
      } else {
        r = kResidualCarry;
        for (int w = wig - 1; w >= 0; --w)
          if (whas[grp * 4 + w]) {
            r = fabsf(wlast[grp * 4 + w]);
            break;
          }
      }
      res = r;
    }
    if (tid < kChainGroups * 16) {
      // publish this evaluation's records (self-contained words, relaxed); only the last evaluation has other data to
      // order before them: the forwardMatch keys this workgroup issued - and waited for - before the __syncthreads above
      const int g = tid >> 4, k = tid & 15;
      unsigned long long* out = xch + ((size_t)(call & 1) * nrec_launched + (size_t)blockIdx.x * kChainGroups + g) * kPartStride;
      const unsigned tag = tag_base + (unsigned)call + 1u;
      if (k < 10) {
        float acc = 0.f;
        for (int w = 0; w < 4; ++w) acc += wsum[g * 4 + w][k];
        xch_publish(out + k, tag, acc);
      } else if (k == 10 || k == 11) {
        float hv = 0.f, lv = 0.f;
        for (int w = 3; w >= 0; --w)
          if (whas[g * 4 + w]) {
            hv = 1.f;
            lv = wlast[g * 4 + w];
            break;
          }
        xch_publish(out + k, tag, k == 10 ? hv : lv);
      }
    }
    __syncthreads();  // wsum / whas / wlast are rewritten by the next evaluation
    RH_STAMP(1 + call * 6 + 5);
  }

  // final accept / reject of minimizeVel (core.cpp:166-185 for the last evaluation)
  if (lm_live && calls > 0) {
    chain_collect_records<kChainThreads>(xch + (size_t)((calls - 1) & 1) * nrec_launched * kPartStride, tag_base + (unsigned)calls, nblocks,
                                         rec, red, carry_in, bar_err, slow_poll);
    if (tid == 0) lm_step(s, red, calls, true);
    __syncthreads();
  }
  if (blockIdx.x == 0 && tid == 0) {
    *st_out = s;
    if (slot) slot_sum = slot_fill(slot, s, nm.st, om.st);  // zero-copy: the host reads these once the stamps say so
  }
  RH_STAMP(1 + calls * 6);
  if (!do_ext) {
    if (slot && blockIdx.x == 0 && tid == 0) {
      slot->sum = slot_sum ^ ga.seq;
      stamp_drain(&slot->seq, ga.seq);
    }
    return;
  }
  if (hist_to_zero && blockIdx.x == 0 && tid < 128) hist_to_zero[tid] = 0;  // every evaluation has consumed the histogram
  if (blockIdx.x == 0 && tid < 3) xch_publish(xch_final + tid, tag_final, s.vel[tid]);
  if (!lm_live) {
    if (tid < 3) s.vel[tid] = xch_wait(xch_final + tid, tag_final, bar_err);
    __syncthreads();
  }
  const float vx = s.vel[0], vy = s.vel[1], vz = s.vel[2];
  float row[6] = {0, 0, 0, 0, 0, 0};
  float Y = 0.f;
  int cnt = 0;
  xch_acquire();  // behind the polls of the last evaluation's records: the forwardMatch keys of every workgroup (vm_drain)
  if (idx < n_new) {
    xk.key = __hip_atomic_load(&nm.fwd_key[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    xrv_eval(p, om, nm, idx, 1, xk, vx, vy, vz, row, &Y, &cnt);
  }
  float v[28];
  {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) v[k++] = row[i] * row[j];
#pragma unroll
    for (int i = 0; i < 6; ++i) v[21 + i] = row[i] * Y;
    v[27] = (float)cnt;
  }
  wave_total63_fN(v);
  if (lane == 63) {
#pragma unroll
    for (int k = 0; k < 28; ++k) wsum[wid][k] = v[k];
  }
  __syncthreads();
  // (both kernels keep the same exchange layout: the extRotVel words follow the speculative kernel's words)
  unsigned long long* xch_xrv = xch + lm_xch_xrv_offset((size_t)nrec_launched, (size_t)gridDim.x);
  if (tid < kChainGroups * 32) {
    const int g = tid >> 5, k = tid & 31;
    unsigned stored = 0u;
    if (k < 28) {
      float acc = 0.f;
      for (int w = 0; w < 4; ++w) acc += wsum[g * 4 + w][k];
      if (ga.lm)
        xch_publish(xch_xrv + ((size_t)blockIdx.x * kChainGroups + g) * kXrvStride + k, tag_final, acc);
      else
        xrv_part[((size_t)blockIdx.x * kChainGroups + g) * kXrvStride + k] = acc;
      stored = __float_as_uint(acc);
    }
    // records that go straight to the host (per-pair API): each carries the pair's sequence stamp in its last word, stored once
    // this wave's 28 sums are acknowledged - a host that polls the records instead of waiting for an event reads complete ones
    if (!ga.lm) xrv_record_stamp(xrv_part + ((size_t)blockIdx.x * kChainGroups + g) * kXrvStride, k, ga.seq, stored);
  }
  RH_STAMP(2 + calls * 6);
  if (ga.lm) {
    __syncthreads();  // (rec is free: every LM collect is over)
    lm_tail_glue<kChainThreads>(ga, xch_xrv, tag_final, n_new, rec, kMaxRecBlocks * kPartStride / kXrvStride, gw, s, bar_err, slow_poll, stamps);
  }
  if (slot && blockIdx.x == 0 && tid == 0) {  // the slot's stamp: by the directedMatch launch with the glue's record, or here
    slot->sum = slot_sum ^ ga.seq;
    if (ga.lm && ga.stage)
      ga.stage->host_slot = slot;
    else
      stamp_drain(&slot->seq, ga.seq);
  }
#undef RH_STAMP
}

// ---- persistent minimizeVel with SPECULATIVE evaluation of the reject chain ------------------------------------------------
// Observation (tools/mask_hist.py, profiles/r02_divergence_report.txt): on every tested stream minimizeVel accepts its first
// step and rejects the other four (accept mask 00001). After a rejection the next trial point depends on nothing the rejected
// evaluation produced: u *= v, v *= 2, h = -(JtJ + uI)^-1 JtF with the OLD JtJ / JtF (core.cpp:180-183). So once the result of
// evaluation 1 is in, the points of evaluations 2, 3, .., calls-1 under the hypothesis "all rejected" are known, and they are
// evaluated back to back in ONE pass - three exchange rounds per launch instead of six. Then the hypothesis is checked with
// the real scores (the gain test of core.cpp:172, same expression); if an evaluation turns out accepted, the launch continues
// from there with ordinary one-evaluation passes (nothing speculative is kept: state and residuals are rolled back to that
// evaluation, the forwardMatch keys the speculative last evaluation published are cleared behind a grid barrier). Either way
// the results are those of the sequential algorithm, bit for bit (test_persistent_lm_kernel_equals_per_call_kernels).
// What consecutive evaluations of one pass need from OTHER workgroups is only the carry-forward of the last written fi
// (oracle header, H3) for keylines in front of their group's first match: each workgroup hands the fi of its last matched
// keyline to its right neighbour through one tagged word per evaluation, published right after the evaluation and polled
// after the workgroup's own reduction (the hop hides behind it).
// Exchange words: [kMaxLmCalls][record groups][kPartStride] record sets (one per evaluation index: no slot is reused within a
// launch), kPartStride words for the final velocity, [kMaxLmCalls][workgroups][2] carry words, [workgroups] barrier words.
// Tags: tag_base + phase * (calls + 1) + evaluation + 1, phase 1 = evaluations repeated after a failed hypothesis; the caller
// advances tag_base by 2 * (calls + 1) per launch.
constexpr int kSpecMax = 6;  // speculative evaluations per launch (iterations <= 7)

template <int kChainThreads>
__device__ __forceinline__ void lm_chain_spec_body(KParams p, MapDev om, MapDev nm, int calls, const LmState* __restrict__ st_in,
                                                   LmState* __restrict__ st_out, unsigned long long* __restrict__ xch, unsigned tag_base,
                                                   int* __restrict__ bar_err, const int* __restrict__ hist, unsigned frame_count,
                                                   float* __restrict__ xrv_part, PairSlot* __restrict__ slot, int* __restrict__ hist_to_zero,
                                                   unsigned long long* __restrict__ stamps, int slow_poll, const GlueArgs ga, int kf) {
  unsigned slot_sum = 0u;  // XOR of the words thread 0 of workgroup 0 stored into the result slot (PairSlot::sum)
  // kf = index of the first speculative evaluation: evaluations 0 .. kf - 1 run one per exchange round, kf .. calls - 1 in one
  // pass under the hypothesis "all rejected". kf = 2: the steady state of a young stream (accept mask 00001); kf = 3: what the
  // same stream settles into once its depths have converged (00011 on every pair from frame ~6000 on) - four
  // exchange rounds instead of the six of k_lm_chain or of a roll-back.
  constexpr int kChainGroups = kChainThreads / 256;
  constexpr int kWaves = kChainThreads / 64;
  __shared__ GlueLds gw;
  __shared__ float lm_inv[4][9];
  // REBVIO_HIP_LM_STAMPS: 1 start, 2/3 evaluations 0/1 published, 4 hypothesis states ready, speculative evaluations: 5 projected,
  // 6 gathers issued, 7 matches known, 8 neighbour round done, 9 weighted sums done, 10 published; 11 all record sets staged and
  // reduced, 12 hypothesis checked, 13 LM done, 14 extRotVel rows out (stamps[0] = 1 marks the layout)
#define RH_STAMP(i) \
  do { if (stamps && blockIdx.x == 0 && threadIdx.x == 0) stamps[(i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
  extern __shared__ float recm[];  // [nspec][cap * kPartStride] staged record sets (set 0 doubles as the ordinary collect's staging)
  __shared__ LmState s;
  __shared__ LmState stc[kSpecMax + 1];  // state before evaluation 2 + k's result is processed (k = 0 .. nspec), under the hypothesis
  __shared__ float red[16];
  __shared__ float redm[kSpecMax][16];
  __shared__ float carry_in[kChainGroups];
  __shared__ float wsum[kWaves][28];
  __shared__ float wlast[kWaves];
  __shared__ int whas[kWaves];
  __shared__ int shist[128];
  __shared__ int first_accept;
  __shared__ float wsumk[kSpecMax][kWaves][10];  // speculative evaluations: per-wave sums, match flags, last fi, carry-in per group
  __shared__ int whask[kSpecMax][kWaves];
  __shared__ float wlastk[kSpecMax][kWaves];
  __shared__ float carryk[kSpecMax + 1][kChainGroups];

  const int tid = threadIdx.x;
  const unsigned long long t_entry = (stamps && blockIdx.x == 0 && tid == 0) ? __builtin_amdgcn_s_memrealtime() : 0ull;  // diagnostic
  const int idx = blockIdx.x * kChainThreads + tid;
  const int lane = tid & 63, wid = tid >> 6, grp = tid >> 8, wig = wid & 3;
  const int nwg = gridDim.x;
  const int nrec_launched = nwg * kChainGroups;
  const TvIn in = make_tvin(p, om.gnorm[idx], om.rs[idx], om.pos_img[idx], om.grad[idx], om.matches[idx]);
  float res = om.residual[idx];
  XrvIn xk{};
  XrvFwd xf{};
  xf.o = -1;
  bool xf_valid = false;  // the forwardMatch gathers of this thread's keyline are in `xf` (issued behind the speculative collect)
  xk.mid = nm.match_id[idx];
  xk.rs = nm.rs[idx];
  xk.mpi = nm.mpos_img[idx];
  xk.g = nm.grad[idx];
  xk.gn = nm.gnorm[idx];
  xk.q = nm.pos_img[idx];
  const int n = om.st->n;
  const float thr = om.st->threshold;
  const int n_new = nm.st->n;
  const int nblocks = (n + 255) / 256;
  const int cap = min(nblocks, kMaxRecBlocks) * kPartStride;  // words staged per record set
  if (tid < 128) shist[tid] = (tid < p.quantile_num_bins) ? hist[tid] : 0;
  if (tid == 0) s = *st_in;
  if (tid < kChainGroups) carry_in[tid] = 0.f;
  __syncthreads();
  const unsigned min_matches = min(p.min_match_threshold, frame_count);
  const bool lm_live = blockIdx.x == 0 || (int)blockIdx.x * kChainGroups < nblocks;
  // Evaluation 0 is taken at the incoming velocity, so its projection and its two dependent gathers (field cell, then the
  // cell's keyline) start before the sigma quantile is known; the quantile's only part in it - the uncertainty gate of
  // tv_project - is applied to the finished projection below (a gated keyline's gathers are never looked at).
  TvProj pj0{};
  pj0.cell = -1;
  pj0.skip = true;
  TvGeo ge0{};
  ge0.id = -1;
  if (lm_live && idx < n) {
    pj0 = tv_project(p, in, s.vel[0], s.vel[1], s.vel[2], __builtin_inff(), thr, min_matches);
    ge0 = tv_geometry(p, nm, tv_cell(nm, pj0));
  }
  if (tid < 64) {
    const float q = quantile_from_hist_wave(shist, p.quantile_num_bins, p.quantile_cutoff, n, tid);
    if (tid == 0) {
      s.sigma_rho_min = q;
      for (int i = 0; i < 3; ++i) s.Vnew[i] = s.vel[i];
    }
  }
  __syncthreads();
  const float srm = s.sigma_rho_min;
  if (in.rs.y > srm) {
    pj0.skip = true;
    pj0.cell = -1;
  }
  const int live_wgs = max(1, (nblocks + kChainGroups - 1) / kChainGroups);
  unsigned long long* xch_final = xch + (size_t)kMaxLmCalls * nrec_launched * kPartStride;
  unsigned long long* xch_carry = xch_final + kPartStride;                  // [kMaxLmCalls][nwg][2]
  unsigned long long* xch_sync = xch_carry + (size_t)kMaxLmCalls * nwg * 2;  // [nwg]
  const unsigned tag_final = tag_base + 2u * ((unsigned)calls + 1u);
  auto tag_of = [&](int call, int phase) { return tag_base + (unsigned)phase * ((unsigned)calls + 1u) + (unsigned)call + 1u; };
  int fa = -1;  // index of the first speculative evaluation that turned out accepted (-1: none / not known yet)
  auto set_words = [&](int call) { return xch + (size_t)call * nrec_launched * kPartStride; };

  // One evaluation at (vx, vy, vz): tryVel body, carry-forward, wave / workgroup sums, records published under `tag`.
  auto do_eval = [&](int call, unsigned tag, const TvProj& pj, const TvGeo& ge, bool last) {
    const float cin = carry_in[grp];
    TvOut e{};
    e.mfwd = -1;
    if (idx < n) {
      e = tv_finish(p, in, pj, ge, res, cin);
      if (e.wrote_res) res = e.res_out;
      if (last) {
        if (e.matched) {
          const unsigned long long key = ((unsigned long long)order_key(in.rs.x) << 32) | (unsigned)idx;
          fwd_key_max(&nm.fwd_key[e.mfwd], key);
        }
        om.match_fwd[idx] = e.mfwd;
      }
    }
    if (last) vm_drain();  // the keys are out before the records (see the speculative phase)
    const unsigned long long mm = __ballot(e.matched);
    const unsigned long long below = mm & ((1ull << lane) - 1ull);
    const int src = below ? (63 - __clzll((long long)below)) : 0;
    const float fi_prev = __shfl(e.fi, src);
    const int wl = mm ? (63 - __clzll((long long)mm)) : 0;
    const float fi_wlast = __shfl(e.fi, wl);
    if (lane == 0) {
      whas[wid] = mm ? 1 : 0;
      wlast[wid] = fi_wlast;
    }
    const float sc = e.contrib ? e.f * e.f : 0.f;
    float v[10] = {sc, e.jx * e.jx, e.jy * e.jy, e.jz * e.jz, e.jx * e.jy, e.jx * e.jz, e.jy * e.jz, e.jx * e.f, e.jy * e.f, e.jz * e.f};
    wave_total63_fN(v);
    if (lane == 63) {
#pragma unroll
      for (int k = 0; k < 10; ++k) wsum[wid][k] = v[k];
    }
    __syncthreads();
    if (e.need_carry) {
      float r;
      if (below) {
        r = fabsf(fi_prev);
      } else {
        r = kResidualCarry;
        for (int w = wig - 1; w >= 0; --w)
          if (whas[grp * 4 + w]) {
            r = fabsf(wlast[grp * 4 + w]);
            break;
          }
      }
      res = r;
    }
    if (tid < kChainGroups * 16) {
      const int g = tid >> 4, k = tid & 15;
      unsigned long long* out = set_words(call) + ((size_t)blockIdx.x * kChainGroups + g) * kPartStride;
      if (k < 10) {
        float acc = 0.f;
        for (int w = 0; w < 4; ++w) acc += wsum[g * 4 + w][k];
        xch_publish(out + k, tag, acc);
      } else if (k == 10 || k == 11) {
        float hv = 0.f, lv = 0.f;
        for (int w = 3; w >= 0; --w)
          if (whas[g * 4 + w]) {
            hv = 1.f;
            lv = wlast[g * 4 + w];
            break;
          }
        xch_publish(out + k, tag, k == 10 ? hv : lv);
      }
    }
    __syncthreads();  // wsum / whas / wlast are rewritten by the next evaluation
  };

  // ordinary collect of one record set (+ carry-in per group) into recm[0 .. cap) / red
  auto collect = [&](int call_of_set, unsigned tag) {
    const unsigned long long* sw = set_words(call_of_set);
    for (int i0 = 0; i0 < cap; i0 += kChainThreads * 2) {  // a thread's two words of a 16k-keyline map polled together
      const int ia = i0 + tid, ib = i0 + kChainThreads + tid;
      const unsigned long long* const w2[2] = {sw + min(ia, cap - 1), sw + min(ib, cap - 1)};
      const unsigned t2[2] = {tag, tag};
      const bool ok2[2] = {ia < cap && (ia & (kPartStride - 1)) < 12, ib < cap && (ib & (kPartStride - 1)) < 12};
      float o2[2];
      xch_wait_many<2>(w2, t2, ok2, o2, bar_err, slow_poll);
      if (ok2[0]) recm[ia] = o2[0];
      if (ok2[1]) recm[ib] = o2[1];
    }
    __syncthreads();
    reduce_staged_records(recm, nblocks, red, carry_in, (int)blockIdx.x * kChainGroups, kChainGroups);
    __syncthreads();
  };
  auto normal_pass = [&](int call, int phase) {
    if (call >= 1) {
      collect(call - 1, tag_of(call - 1, (phase == 1 && call - 1 >= fa + kf + 1) ? 1 : 0));
      if (tid < 64) lm_step_wave(s, red, call, false, lm_inv[0], tid);
      __syncthreads();
    }
    TvProj pj{};
    TvGeo ge{};
    if (idx < n) {
      pj = tv_project(p, in, s.Vnew[0], s.Vnew[1], s.Vnew[2], srm, thr, min_matches);
      ge = tv_geometry(p, nm, tv_cell(nm, pj));
    }
    do_eval(call, tag_of(call, phase), pj, ge, call == calls - 1);
  };

  const int nspec = calls - kf;  // evaluations kf .. calls - 1 (the launcher guarantees 2 <= nspec <= kSpecMax)
  // diagnostic: from the end of the previous launch (its last stamp) to the start of this one = the pair's second half with
  // every stream operation between the kernels; summed on the device (the launches of a stream are serialised)
  if (stamps && blockIdx.x == 0 && tid == 0) {
    const unsigned long long now = __builtin_amdgcn_s_memrealtime(), prev_end = stamps[15];
    if (stamps[0] == 1ull && prev_end != 0ull && now > prev_end && now - prev_end < 100000ull) {
      stamps[40] += now - prev_end;
      stamps[41] += 1ull;
      const unsigned long long g0 = stamps[14], g1 = stamps[16], g2 = stamps[17], g3 = stamps[18];
      if (g1 > g0 && g2 > g1 && g3 >= g2 && prev_end > g3) {  // glue of the previous launch: sums in, solve done, all waves done, end
        stamps[51] += g1 - g0;
        stamps[52] += g2 - g1;
        stamps[53] += g3 - g2;
        stamps[54] += prev_end - g3;
        stamps[55] += 1ull;
      }
      const unsigned long long t1 = stamps[48], t2 = stamps[49], t3 = stamps[50];
      if (t1 > prev_end && t2 > t1 && t3 > t2 && now > t3) {  // start of the head, the tail, regularize / EKF of that pair
        stamps[42] += t1 - prev_end;
        stamps[43] += t2 - t1;
        stamps[44] += t3 - t2;
        stamps[45] += now - t3;
        stamps[46] += 1ull;
        stamps[56] += now - t_entry;  // kernel entry -> here: the keyline loads and the sigma quantile ahead of the first evaluation
      }
    }
  }
  RH_STAMP(1);
  if (lm_live) {
    do_eval(0, tag_of(0, 0), pj0, ge0, false);  // (calls >= kf + 2: evaluation 0 is never the last one)
    RH_STAMP(2);
    for (int call = 1; call < kf; ++call) normal_pass(call, 0);
    RH_STAMP(3);
    collect(kf - 1, tag_of(kf - 1, 0));
    // the real step and the first three states under the hypothesis in one go (lm_step_wave_states)
    if (tid < 64) lm_step_wave_states(s, red, kf, lm_inv, tid, stc, min(nspec, 4));
    __syncthreads();
    // further states under the hypothesis (iterations > 5): state g + 1 applies g rejections' (u, v) updates and then one
    // lm_step whose score is NaN (the gain test fails for any denominator): exactly the reject branch of core.cpp:180-183
    // plus the next trial point. Sixteen lanes per state, nine of them with one cofactor of its 3x3 inverse each.
    for (int g0 = 3; g0 < nspec - 1; g0 += 4) {
      if (tid < 64) {
        const int g = g0 + (tid >> 4), e = tid & 15;
        const bool act = g < nspec - 1;
        LmState t = s;
        for (int j = 0; j < g; ++j) {
          t.u *= t.v;
          t.v = (float)((double)t.v * 2.0);
        }
        float fake[10];
#pragma unroll
        for (int i = 0; i < 10; ++i) fake[i] = __uint_as_float(0x7FC00000u);
        lm_step_book(t, fake, kf + 1 + g);
        float M[9];
        lm_step_matrix(t, M);
        const float d = glue_det3(M);
        float o;
        switch (e) {
          case 0: o = M[4] * M[8] - M[5] * M[7]; break;
          case 1: o = M[2] * M[7] - M[1] * M[8]; break;
          case 2: o = M[1] * M[5] - M[2] * M[4]; break;
          case 3: o = M[5] * M[6] - M[3] * M[8]; break;
          case 4: o = M[0] * M[8] - M[2] * M[6]; break;
          case 5: o = M[2] * M[3] - M[0] * M[5]; break;
          case 6: o = M[3] * M[7] - M[4] * M[6]; break;
          case 7: o = M[1] * M[6] - M[0] * M[7]; break;
          default: o = M[0] * M[4] - M[1] * M[3]; break;
        }
        glue_wave_sync();
        if (act && e < 9) lm_inv[tid >> 4][e] = o / d;
        glue_wave_sync();
        if (act && e == 0) {
          float inv[9];
#pragma unroll
          for (int i = 0; i < 9; ++i) inv[i] = lm_inv[tid >> 4][i];
          lm_step_apply(t, inv);
          stc[g + 1] = t;
        }
        glue_wave_sync();
      }
    }
    __syncthreads();
    RH_STAMP(4);
    // the gathers of all speculative evaluations in flight together: projections (no memory), then every field cell, then
    // every matched keyline's geometry; what remains per evaluation is arithmetic and the workgroup / neighbour hand-offs
    TvProj pj[kSpecMax];
    unsigned cellkey[kSpecMax];
    TvGeo ge[kSpecMax];
#pragma unroll
    for (int k = 0; k < kSpecMax; ++k) {
      pj[k] = TvProj{};
      pj[k].cell = -1;
      pj[k].skip = true;
      if (k < nspec && idx < n) pj[k] = tv_project(p, in, stc[k].Vnew[0], stc[k].Vnew[1], stc[k].Vnew[2], srm, thr, min_matches);
    }
    RH_STAMP(5);
#pragma unroll
    for (int k = 0; k < kSpecMax; ++k) cellkey[k] = tv_cell(nm, pj[k]);
#pragma unroll
    for (int k = 0; k < kSpecMax; ++k) ge[k] = tv_geometry(p, nm, cellkey[k]);
    // What an evaluation hands to the next one - who matched, the last written fi - does not depend on the residuals, so it is
    // settled for ALL speculative evaluations first: one workgroup barrier and one neighbour round instead of one per
    // evaluation. After that the residual / weight chain of a keyline is arithmetic on its own registers.
    RH_STAMP(6);
    TvMatch mt[kSpecMax];
    float rcarry[kSpecMax];  // residual an unmatched keyline ends evaluation k with (|fi| of the last match before it, or the marker)
#pragma unroll
    for (int k = 0; k < kSpecMax; ++k) {
      mt[k] = tv_match(p, in, pj[k], ge[k]);
      rcarry[k] = kResidualCarry;
      if (k < nspec) {
        const unsigned long long mm = __ballot(mt[k].matched);
        const unsigned long long below = mm & ((1ull << lane) - 1ull);
        const float fi_prev = __shfl(mt[k].fi, below ? (63 - __clzll((long long)below)) : 0);
        const float fi_wlast = __shfl(mt[k].fi, mm ? (63 - __clzll((long long)mm)) : 0);
        if (below) rcarry[k] = fabsf(fi_prev);
        if (lane == 0) {
          whask[k][wid] = mm ? 1 : 0;
          wlastk[k][wid] = fi_wlast;
        }
        if (kf + k == calls - 1 && idx < n) {  // the side effects of the last evaluation (forwardMatch, edge_map.cpp:78-96)
          if (mt[k].matched) {
            const unsigned long long key = ((unsigned long long)order_key(in.rs.x) << 32) | (unsigned)idx;
            fwd_key_max(&nm.fwd_key[mt[k].mfwd], key);
          }
          om.match_fwd[idx] = mt[k].mfwd;
        }
      }
    }
    // (the forwardMatch atomics issued above stay in flight through the neighbour round and the weighted sums; they are
    // waited for in front of the barrier the record sets are published behind)
    RH_STAMP(7);
    __syncthreads();
    // thread kChainThreads - 1 - k: hand-off behind evaluation kf + k (carry-in of evaluation kf + 1 + k), as in do_eval
    if (tid >= kChainThreads - (nspec - 1)) {
      const int k = kChainThreads - 1 - tid;
      const int call = kf + k;
      const unsigned tag = tag_of(call, 0);
      int own_has = 0;
      float own_last = 0.f;
      for (int w = kWaves - 1; w >= 0; --w)
        if (whask[k][w]) {
          own_has = 1;
          own_last = wlastk[k][w];
          break;
        }
      unsigned long long* cw = xch_carry + ((size_t)call * nwg + blockIdx.x) * 2;
      if (own_has && (int)blockIdx.x + 1 < live_wgs) {
        xch_publish(cw, tag, 1.0f);
        xch_publish(cw + 1, tag, own_last);
      }
      float in_has = 0.f, in_fi = 0.f;
      if (blockIdx.x > 0) {
        const unsigned long long* lw = xch_carry + ((size_t)call * nwg + (blockIdx.x - 1)) * 2;
        in_has = xch_wait(lw, tag, bar_err, slow_poll);
        in_fi = xch_wait(lw + 1, tag, bar_err, slow_poll);
      }
      if (!own_has && (int)blockIdx.x + 1 < live_wgs) {
        xch_publish(cw, tag, in_has);
        xch_publish(cw + 1, tag, in_fi);
      }
      float c = (in_has != 0.f) ? fabsf(in_fi) : 0.f;
      for (int g = 0; g < kChainGroups; ++g) {
        carryk[k + 1][g] = c;
        for (int w = 3; w >= 0; --w)
          if (whask[k][g * 4 + w]) {
            c = fabsf(wlastk[k][g * 4 + w]);
            break;
          }
      }
    }
    if (tid < kChainGroups) carryk[0][tid] = carry_in[tid];  // evaluation kf: from the records of evaluation kf - 1 (collect above)
    __syncthreads();
    RH_STAMP(8);
    float res_hist[kSpecMax];
#pragma unroll
    for (int k = 0; k < kSpecMax; ++k) {
      if (k < nspec) {
        TvOut e{};
        if (idx < n) {
          e = tv_weight(p, in, pj[k], mt[k], res, carryk[k][grp]);
          if (e.wrote_res) res = e.res_out;
        }
        if (mt[k].need_carry) {  // (false for idx >= n: those never pass tv_project)
          float r = rcarry[k];
          if (r == kResidualCarry) {
            for (int w = wig - 1; w >= 0; --w)
              if (whask[k][grp * 4 + w]) {
                r = fabsf(wlastk[k][grp * 4 + w]);
                break;
              }
          }
          res = r;
        }
        res_hist[k] = res;
        const float sc = e.contrib ? e.f * e.f : 0.f;
        float v[10] = {sc, e.jx * e.jx, e.jy * e.jy, e.jz * e.jz, e.jx * e.jy, e.jx * e.jz, e.jy * e.jz, e.jx * e.f, e.jy * e.f, e.jz * e.f};
        wave_total63_fN(v);
        if (lane == 63) {
#pragma unroll
          for (int q = 0; q < 10; ++q) wsumk[k][wid][q] = v[q];
        }
      }
    }
    // Every wave's forwardMatch atomics (performed at the memory side, device scope) are ACKNOWLEDGED before the workgroup goes
    // on to publish its records: vmcnt(0) here, on the waves that issued them, in front of the barrier. (A system-scope release
    // fence on the publishing threads orders only THEIR OWN operations and writes the XCD's whole L2 back for it.)
    vm_drain();
    RH_STAMP(9);
    __syncthreads();
    if (tid < kChainGroups * 16) {
      const int g = tid >> 4, q = tid & 15;
      for (int k = 0; k < nspec; ++k) {
        const int call = kf + k;
        const unsigned tag = tag_of(call, 0);
        unsigned long long* out = set_words(call) + ((size_t)blockIdx.x * kChainGroups + g) * kPartStride;
        if (q < 10) {
          float acc = 0.f;
          for (int w = 0; w < 4; ++w) acc += wsumk[k][g * 4 + w][q];
          xch_publish(out + q, tag, acc);
        } else if (q == 10 || q == 11) {
          float hv = 0.f, lv = 0.f;
          for (int w = 3; w >= 0; --w)
            if (whask[k][g * 4 + w]) {
              hv = 1.f;
              lv = wlastk[k][g * 4 + w];
              break;
            }
          xch_publish(out + q, tag, q == 10 ? hv : lv);
        }
      }
    }
    __syncthreads();  // (the roll-back path reuses the staging arrays)
    RH_STAMP(10);
    // all nspec record sets at once: every thread first issues its loads together, then waits for the stragglers
    {
      const int total = nspec * cap;
      for (int i0 = 0; i0 < total; i0 += kChainThreads * 8) {
        const unsigned long long* w8[8];
        unsigned t8[8];
        bool ok8[8];
        float o8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int i = min(i0 + j * kChainThreads + tid, total - 1);
          const int set = i / cap, w = i - set * cap;
          ok8[j] = i0 + j * kChainThreads + tid < total && (w & (kPartStride - 1)) < 12;
          w8[j] = set_words(kf + set) + w;
          t8[j] = tag_of(kf + set, 0);
        }
        xch_wait_many<8>(w8, t8, ok8, o8, bar_err, slow_poll);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (ok8[j]) recm[i0 + j * kChainThreads + tid] = o8[j];
      }
      __syncthreads();
      // Every workgroup's record sets are in, hence every forwardMatch key of the last evaluation (vm_drain above): this
      // keyline's key is fetched HERE, under the hypothesis, and returns while the sums are reduced and checked; the gathers
      // through it follow the check (below) and return while the state is finished.
      xch_acquire();
      if (idx < n_new) xk.key = __hip_atomic_load(&nm.fwd_key[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (int set0 = 0; set0 < nspec; set0 += kChainThreads / 160) {
        const int sl = tid / 160, set = set0 + sl;
        if (sl < kChainThreads / 160 && set < nspec) reduce_staged_sums(recm + (size_t)set * cap, nblocks, redm[set], sl * 160);
      }
      __syncthreads();
    }
    RH_STAMP(11);
    // the hypothesis against the real scores: the gain test of core.cpp:172 on the state the evaluation started from
    {
      bool accepted = false;
      if (tid < nspec) {
        const LmState& t = stc[tid];
        const float Fnew = redm[tid][0];
        double den = 0.0;
        for (int i = 0; i < 3; ++i) den += (0.5 * (double)t.h[i]) * (double)(t.u * t.h[i] - t.JtF[i]);
        const float gain = (float)((double)(t.F - Fnew) / den);
        accepted = gain > 0.0f;
      }
      if (wid == 0) {
        const unsigned long long am = __ballot(accepted);
        if (lane == 0) first_accept = am ? (__ffsll((long long)am) - 1) : -1;
      }
      __syncthreads();
    }
    fa = first_accept;
    RH_STAMP(12);
    if (fa < 0 || fa == nspec - 1) {  // the keys of the speculative last evaluation stand
      if (idx < n_new) xf = xrv_gather(om, xk.key);
      xf_valid = true;
    }
    if (fa < 0) {
      if (tid == 0) {  // every evaluation rejected: the last rejection is the final step of core.cpp:166-185 (no new trial point)
        LmState t = stc[nspec - 1];
        t.u *= t.v;
        t.v = (float)((double)t.v * 2.0);
        s = t;
      }
      __syncthreads();
    } else {
      // evaluation kf + fa was accepted: go on from there the ordinary way. Roll back, clear the keys the speculative last
      // evaluation published, and let nobody publish a repeated evaluation before everybody has read the speculative sets.
      __atomic_thread_fence(__ATOMIC_ACQUIRE);  // the keys other workgroups issued before their last record set
      if (tid == 0) s = stc[fa];
#pragma unroll
      for (int k = 0; k < kSpecMax; ++k)
        if (k == fa) res = res_hist[k];
      // (fa == nspec - 1: the accepted evaluation is the last one - its trial point was the real one, its keys stand)
      if (fa < nspec - 1)
        for (int i = blockIdx.x * kChainThreads + tid; i < p.kmax; i += live_wgs * kChainThreads) nm.fwd_key[i] = 0ull;
      __syncthreads();
      if (tid == 0) {
        __atomic_thread_fence(__ATOMIC_RELEASE);
        xch_publish(xch_sync + blockIdx.x, tag_final, 1.0f);
      }
      for (int i = tid; i < live_wgs; i += kChainThreads) (void)xch_wait(xch_sync + i, tag_final, bar_err, slow_poll);
      __syncthreads();
      __atomic_thread_fence(__ATOMIC_ACQUIRE);
      for (int call = kf + 1 + fa; call < calls; ++call) normal_pass(call, 1);
      collect(calls - 1, tag_of(calls - 1, (calls - 1 >= fa + kf + 1) ? 1 : 0));
      if (tid == 0) lm_step(s, red, calls, true);
      __syncthreads();
    }
  }
  // The final state and the pair's result slot (zero-copy: the host reads them once the stamps say so) are written by the LAST
  // live workgroup, behind its extRotVel records: every live workgroup holds the same state, and workgroup 0, which goes on
  // to the device glue and is waited for by it, no longer spends a microsecond of a lone thread's stores in front of its rows.
  const int fill_wg = live_wgs - 1;
  RH_STAMP(13);
  if (hist_to_zero && blockIdx.x == 0 && tid < 128) hist_to_zero[tid] = 0;  // every evaluation has consumed the histogram
  if (blockIdx.x == 0 && tid < 3) xch_publish(xch_final + tid, tag_final, s.vel[tid]);
  if (!lm_live) {
    if (tid < 3) s.vel[tid] = xch_wait(xch_final + tid, tag_final, bar_err, slow_poll);
    __syncthreads();
  }
  const float vx = s.vel[0], vy = s.vel[1], vz = s.vel[2];
  float row[6] = {0, 0, 0, 0, 0, 0};
  float Y = 0.f;
  int cnt = 0;
  if (!xf_valid) {  // (workgroups without LM work, or after a roll-back)
    xch_acquire();  // behind the polls of the last evaluation's records: the forwardMatch keys of every workgroup (vm_drain)
    if (idx < n_new) {
      xk.key = __hip_atomic_load(&nm.fwd_key[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      xf = xrv_gather(om, xk.key);
    }
  }
  if (idx < n_new) xrv_apply(p, nm, idx, 1, xf, xk, vx, vy, vz, row, &Y, &cnt);
  float v[28];
  {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) v[k++] = row[i] * row[j];
#pragma unroll
    for (int i = 0; i < 6; ++i) v[21 + i] = row[i] * Y;
    v[27] = (float)cnt;
  }
  wave_total63_fN(v);
  if (lane == 63) {
#pragma unroll
    for (int k = 0; k < 28; ++k) wsum[wid][k] = v[k];
  }
  __syncthreads();
  unsigned long long* xch_xrv = xch + lm_xch_xrv_offset((size_t)nrec_launched, (size_t)nwg);
  if (tid < kChainGroups * 32) {
    const int g = tid >> 5, k = tid & 31;
    unsigned stored = 0u;
    if (k < 28) {
      float acc = 0.f;
      for (int w = 0; w < 4; ++w) acc += wsum[g * 4 + w][k];
      if (ga.lm)
        xch_publish(xch_xrv + ((size_t)blockIdx.x * kChainGroups + g) * kXrvStride + k, tag_final, acc);
      else
        xrv_part[((size_t)blockIdx.x * kChainGroups + g) * kXrvStride + k] = acc;
      stored = __float_as_uint(acc);
    }
    // records that go straight to the host (per-pair API): each carries the pair's sequence stamp in its last word, stored once
    // this wave's 28 sums are acknowledged - a host that polls the records instead of waiting for an event reads complete ones
    if (!ga.lm) xrv_record_stamp(xrv_part + ((size_t)blockIdx.x * kChainGroups + g) * kXrvStride, k, ga.seq, stored);
  }
  RH_STAMP(14);
  if ((int)blockIdx.x == fill_wg && tid == 0) {
    *st_out = s;
    if (slot) slot_sum = slot_fill(slot, s, nm.st, om.st);
  }
  if (stamps && blockIdx.x == 0 && tid == 0) {
    stamps[15] = stamps[14];  // (no device glue in this launch: a zero-length last segment)
    stamps[0] = 1ull;
  }
  if (ga.lm) {
    __syncthreads();  // (recm is free: every LM collect is over)
    // recm holds (calls - 2) record sets of 16 words per launched group: at least 32 floats per group
    lm_tail_glue<kChainThreads>(ga, xch_xrv, tag_final, n_new, recm, (calls - 2) * (cap / kPartStride) * kPartStride / kXrvStride > 0
                                    ? (calls - 2) * (cap / kPartStride) * kPartStride / kXrvStride : 1, gw, s, bar_err, slow_poll, stamps);
    RH_STAMP(15);
  }
  if (slot && (int)blockIdx.x == fill_wg && tid == 0) {  // the slot's stamp: by the directedMatch launch with the glue's record, or here
    slot->sum = slot_sum ^ ga.seq;
    if (ga.lm && ga.stage)
      ga.stage->host_slot = slot;
    else
      stamp_drain(&slot->seq, ga.seq);
  }
#undef RH_STAMP
}

template <int kChainThreads>
__global__ __launch_bounds__(kChainThreads) void k_lm_chain_spec(KParams p, MapDev om, MapDev nm, int calls, const LmState* __restrict__ st_in,
                                                                 LmState* __restrict__ st_out, unsigned long long* __restrict__ xch,
                                                                 unsigned tag_base, int* __restrict__ bar_err, const int* __restrict__ hist,
                                                                 float* __restrict__ xrv_part, PairSlot* __restrict__ slot,
                                                                 int* __restrict__ hist_to_zero, unsigned long long* __restrict__ stamps,
                                                                 GlueArgs ga, int kf) {
  lm_chain_spec_body<kChainThreads>(p, om, nm, calls, st_in, st_out, xch, tag_base, bar_err, hist, 0u, xrv_part, slot, hist_to_zero, stamps,
                                    0, ga, kf);
}
template <int kChainThreads>
__global__ __launch_bounds__(kChainThreads) void k_lm_chain_spec_b(KParams p, const LaneStatic* __restrict__ ls,
                                                                   const MapDev* __restrict__ maptab, LaneDynB dyn, int calls, int slow_poll,
                                                                   GlueParams gp, LaneGyroB gyro, int lane0, int kf) {
  const int lane = lane0 + (int)blockIdx.z;  // a launch carries the lanes that fit the device together (launch_lm_chain_b)
  const LaneStatic& L = ls[lane];
  const LaneDyn d = dyn.v[lane];
  PairSlot* slot = gptr(L.slot[d.slot]);
  lm_chain_spec_body<kChainThreads>(p, global_map(lane_map(maptab, lane, d.om, d.om_swap)), global_map(lane_map(maptab, lane, d.nm, d.nm_swap)), calls,
                                    gptr(L.lm_zero), gptr(L.lm) + calls + 1, gptr(L.lm_xch), d.tag_base, gptr(L.lm_bar_err), gptr(L.hist), 0u, gptr(L.xrv_part), slot, gptr(L.hist),
                                    nullptr, slow_poll, lane_glue_args(L, d, calls, gp, gyro.R_next[lane]), kf);
}

template <int kChainThreads>
__global__ __launch_bounds__(kChainThreads) void k_lm_chain(KParams p, MapDev om, MapDev nm, int calls, int do_ext,
                                                            const LmState* __restrict__ st_in, LmState* __restrict__ st_out,
                                                            unsigned long long* __restrict__ xch, unsigned tag_base,
                                                            int* __restrict__ bar_err, const int* __restrict__ hist,
                                                            unsigned frame_count, float* __restrict__ xrv_part,
                                                            PairSlot* __restrict__ slot, int* __restrict__ hist_to_zero,
                                                            unsigned long long* __restrict__ stamps, GlueArgs ga) {
  lm_chain_body<kChainThreads>(p, om, nm, calls, do_ext, st_in, st_out, xch, tag_base, bar_err, hist, frame_count, xrv_part, slot,
                               hist_to_zero, stamps, 0, ga);
}
// batched form (lane = blockIdx.z): every lane's workgroups exchange records among themselves through the lane's own words
template <int kChainThreads>
__global__ __launch_bounds__(kChainThreads) void k_lm_chain_b(KParams p, const LaneStatic* __restrict__ ls,
                                                              const MapDev* __restrict__ maptab, LaneDynB dyn, int calls, int slow_poll,
                                                              GlueParams gp, LaneGyroB gyro, int lane0) {
  const int lane = lane0 + (int)blockIdx.z;  // a launch carries the lanes that fit the device together (launch_lm_chain_b)
  const LaneStatic& L = ls[lane];
  const LaneDyn d = dyn.v[lane];
  PairSlot* slot = gptr(L.slot[d.slot]);
  lm_chain_body<kChainThreads>(p, global_map(lane_map(maptab, lane, d.om, d.om_swap)), global_map(lane_map(maptab, lane, d.nm, d.nm_swap)), calls, 1,
                               gptr(L.lm_zero), gptr(L.lm) + calls + 1, gptr(L.lm_xch), d.tag_base, gptr(L.lm_bar_err), gptr(L.hist), 0u, gptr(L.xrv_part), slot, gptr(L.hist), nullptr,
                               slow_poll, lane_glue_args(L, d, calls, gp, gyro.R_next[lane]));
}

// The device glue behind the per-call kernels (REBVIO_HIP_LM=percall): one workgroup; the extRotVel records are in memory
// (kernel boundary), summed in group order in double like hm::sum_xrv.
__global__ __launch_bounds__(256) void k_pair_glue(MapDev nm, GlueArgs ga) {
  __shared__ GlueLds gw;
  __shared__ LmState s;
  const int tid = threadIdx.x;
  if (tid == 0) s = *ga.lm;
  const int nb = (nm.st->n + 255) / 256;
  if (tid < 27) {
    double acc = 0.0;
    for (int b = 0; b < nb; ++b) acc += (double)ga.xrv[(size_t)b * kXrvStride + tid];
    if (tid < 21) {
      int i = 0, base = 0;
      while (tid >= base + (6 - i)) {
        base += 6 - i;
        ++i;
      }
      const int j = i + (tid - base);
      gw.W[i * 6 + j] = (float)acc;
      gw.W[j * 6 + i] = (float)acc;
    } else {
      gw.JtF[tid - 21] = (float)acc;
    }
  }
  __syncthreads();
  glue_workgroup(gw, s, ga);
}
void launch_pair_glue(hipStream_t s, const MapDev& newm, const GlueArgs& ga) { RH_LAUNCH(k_pair_glue, dim3(1), dim3(256), 0, s, newm, ga); }

// ---- EdgeMap::directedMatch / searchMatch (edge_map.cpp:101-218) ----------------------------------------------
// Probe geometry of one query keyline (edge_map.cpp:104-147): everything up to the probe loop.
struct SearchSetup {
  float t_x, t_y, norm_t, pi0x, pi0y, sigma2_t, dq_min, dq_max, dq_rho;
  int t_steps;
};

__device__ __forceinline__ SearchSetup search_setup(const KParams& p, float2 pi, float2 rsq, float2 gq, float gnq,
                                                    const Vec3& vel, const Mat3& Rvel, const Mat3& Rback, float max_radius) {
  SearchSetup S;
  float p_m3[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float s = 0.f;
    s += Rback.a[i * 3 + 0] * pi.x;
    s += Rback.a[i * 3 + 1] * pi.y;
    s += Rback.a[i * 3 + 2] * p.fm;
    p_m3[i] = s;
  }
  const float pmx = p_m3[0] * p.fm / p_m3[2];
  const float pmy = p_m3[1] * p.fm / p_m3[2];
  const float k_rho = rsq.x * p.fm / p_m3[2];
  S.pi0x = pmx + p.cx;
  S.pi0y = pmy + p.cy;
  float t_x = -(vel.a[0] * p.fm - vel.a[2] * pmx);
  float t_y = -(vel.a[1] * p.fm - vel.a[2] * pmy);
  float norm_t = sqrtf(t_x * t_x + t_y * t_y);
  const float DrDv[3] = {p.fm, p.fm, -(pmx + pmy)};
  float rowv[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    float s = 0.f;
    s += DrDv[0] * Rvel.a[0 * 3 + j];
    s += DrDv[1] * Rvel.a[1 * 3 + j];
    s += DrDv[2] * Rvel.a[2 * 3 + j];
    rowv[j] = s;
  }
  float sigma2_t = 0.f;
  sigma2_t += rowv[0] * DrDv[0];
  sigma2_t += rowv[1] * DrDv[1];
  sigma2_t += rowv[2] * DrDv[2];
  S.sigma2_t = sigma2_t;
  // std::max / std::min on NaN operands keep the first argument when the comparison is false; fmaxf/fminf return the
  // non-NaN one. The operands here are finite whenever rho/sigma are, which the depth filter guarantees (core.cpp:451-455).
  if ((double)norm_t > 1e-6) {
    t_x /= norm_t;
    t_y /= norm_t;
    S.dq_rho = norm_t * k_rho;
    S.dq_min = fmaxf(0.0f, norm_t * (k_rho - rsq.y)) - p.pixel_uncertainty_match;
    S.dq_max = fminf(max_radius, norm_t * (k_rho + rsq.y)) + p.pixel_uncertainty_match;
    if (S.dq_rho > S.dq_max) {
      S.dq_rho = (float)(0.5 * (double)(S.dq_max + S.dq_min));
      S.t_steps = cvtt_f64((double)S.dq_rho + 0.5);
    } else {
      S.t_steps = cvtt_f32(fmaxf(S.dq_max - S.dq_rho, S.dq_rho - S.dq_min));
    }
  } else {
    t_x = gq.x;
    t_y = gq.y;
    norm_t = gnq;
    t_x /= norm_t;
    t_y /= norm_t;
    norm_t = 1.0f;
    S.dq_min = -max_radius - p.pixel_uncertainty_match;
    S.dq_max = max_radius + p.pixel_uncertainty_match;
    S.dq_rho = 0.0f;
    S.t_steps = cvtt_f32(S.dq_max);
  }
  S.t_x = t_x;
  S.t_y = t_y;
  S.norm_t = norm_t;
  return S;
}

// Acceptance test of one candidate (edge_map.cpp:170-177)
__device__ __forceinline__ bool search_accept(const KParams& p, const SearchSetup& S, float t, float2 cg, float cgn, float2 crs,
                                              float2 gq, float gnq) {
  const float cang = (cg.x * gq.x + cg.y * gq.y) / (cgn * gnq);
  if (cang < p.cang_min_edge || fabs((double)(cgn / gnq) - 1.0) > (double)p.match_threshold_norm) return false;
  const float v_rho_dr = (p.pixel_uncertainty_match * p.pixel_uncertainty_match + crs.y * crs.y * S.norm_t * S.norm_t +
                          S.sigma2_t * crs.x * crs.x);
  if ((t - S.norm_t * crs.x) * (t - S.norm_t * crs.x) > v_rho_dr) return false;
  return true;
}

// Old-map keyline as directedMatch sees it: stored fields, or (rot != 0) rotated on the fly by R0 - the second
// rotateKeylines of rebvio.cpp:232 folded into the match (the old map is dead afterwards, rebvio.cpp:126-127).
struct OldKl {
  float2 pi, rs, g;
  float gn;
  unsigned matches;  // fetched with the rest (same gather round trip) so that the commit of the accepted candidate does
  int kf;            // not start another one
};
__device__ __forceinline__ OldKl load_old(const MapDev& om, int i, int rot, const Mat3& R0, float fm) {
  OldKl k;
  k.pi = om.pos_img[i];
  k.rs = om.rs[i];
  k.g = om.grad[i];
  k.gn = om.gnorm[i];
  k.matches = om.matches[i];
  k.kf = om.match_kf[i];
  if (rot) rotate_one(R0, fm, k.pi, k.rs, k.g);
  return k;
}

__device__ __forceinline__ void search_commit(MapDev& nm, const MapDev& om, int idx, int found, const OldKl& k, int* kf) {
  (void)om;
  nm.rs[idx] = k.rs;
  nm.match_id[idx] = found;
  nm.matches[idx] = k.matches + 1u;
  nm.mpos_img[idx] = k.pi;
  nm.mgrad[idx] = k.g;
  nm.mgnorm[idx] = k.gn;
  nm.match_kf[idx] = k.kf;
  *kf = (k.kf >= 0) ? 1 : 0;
}

constexpr int kHeadSteps = 4;  // probe steps (2 probes each) of the head of a search: what most keylines are settled in

// vel / Rvel are already rotated by Rback on the host (edge_map.cpp:193-194).
// gd != null: vel / Rvel / Rback / R0 come from *gd (uniform scalar loads) instead of the kernel arguments.
struct DmArgs {
  Vec3 vel;
  Mat3 Rvel, Rback, R0;
  int rot;
  bool skip;
};
__device__ __forceinline__ DmArgs dm_args(const GlueDev* __restrict__ gd, const Vec3& vel, const Mat3& Rvel, const Mat3& Rback, int rot,
                                          const Mat3& R0) {
  DmArgs a;
  if (gd) {
#pragma unroll
    for (int i = 0; i < 3; ++i) a.vel.a[i] = gd->vel_r[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      a.Rvel.a[i] = gd->Rvel_r[i];
      a.Rback.a[i] = gd->Rgva[i];
      a.R0.a[i] = gd->R0a[i];
    }
    a.rot = 1;
    a.skip = gd->nan_v != 0;
  } else {
    a.vel = vel;
    a.Rvel = Rvel;
    a.Rback = Rback;
    a.R0 = R0;
    a.rot = rot;
    a.skip = false;
  }
  return a;
}

// ---- directedMatch (round 4): ONE launch, dense lanes in every expensive phase -----------------------------------------------
// The two-launch forms of rounds 1-3 (a head kernel with one thread or eight lanes per keyline for the first four probe steps,
// a queue of the searches still open, a tail kernel with one wave per queued search; removed, DESIGN.md 6e has their numbers)
// spent most of their instructions on mostly idle lanes: a probe finds a keyline of the old map on
// ~5 % of the pixels it looks at (1.5 of the eight head probes of a keyline, 2 of a long search's ~35), yet the candidate
// fetch + second rotateKeylines + acceptance test (six IEEE divisions, a double-accumulated 3x3 product: ~350 instructions)
// runs once per probe SLOT of the wave, and the long searches take a second launch whose waves hold one keyline each behind
// a queue. Here a wave owns 64 / kLPK keylines of the new map through the whole of searchMatch (edge_map.cpp:101-184), kLPK
// lanes per keyline:
//   phase 1  the kLPK lanes of a keyline share the first kHeadSteps steps (2 * kHeadSteps / kLPK independent mask loads per
//            lane); the wave's candidates are COMPACTED into an LDS list {old keyline, owner, slot} and tested 64 at a time,
//            one candidate per lane; an accepted candidate bids for its owner with an LDS atomicMin on (slot, list position):
//            the smallest slot index is the reference's first hit; the winner's rotated fields are staged per owner in LDS and
//            committed by the owner's first lane.
//   phase 2  the keylines still open after that (long searches: t_steps > kHeadSteps, nothing accepted; 2 600 of 15 000 in the
//            steady state, mean t_steps 20) are searched up to kDmcOpen at a time: two lanes of each walk the reference's two
//            +-1.0f chains (edge_map.cpp:149-150: repeated ++tp / --tn, not dq_rho +- k) into LDS, then ALL 64 lanes share the
//            batch's probe slots, the candidates are compacted and tested as in phase 1.
// Testing every candidate of a keyline instead of stopping at the first accepted one changes nothing (the minimum slot wins)
// and costs little: the tests are what is dense now. Everything is wave-local (no workgroup barrier before the counters).
// kLPK = 4 is the low-latency choice of one stream (938 waves of 16 keylines: a wave's long searches fit one batch - the
// 64-keyline form measured 29 us for phase 2 because waves with 40+ open keylines search them 16 at a time, one after the other);
// kLPK = 1 executes the fewest instructions (batches, large maps).
constexpr int kDmcWin = 40;        // probe steps per long-search window
constexpr int kDmcWinPitch = 41;   // LDS pitch of one chain window (odd: the owners' rows start in different banks)
constexpr int kDmcOpen = 16;       // open keylines a wave searches together (fewer where it owns fewer)
constexpr int kDmcNone = 0x7fffffff;
template <int kKPW, int kBatch>  // keylines per wave (owners), open keylines searched together
struct DmcWave {
  static constexpr int kList = (kBatch * 2 * kDmcWin > kKPW * 2 * kHeadSteps) ? kBatch * 2 * kDmcWin : kKPW * 2 * kHeadSteps;
  unsigned list[kList];              // candidate: old keyline (16 bits) | owner (6) | slot in the reference's probe order, 2 * step + side (10)
  float t1[kKPW * 2 * kHeadSteps];   // phase 1: t of the candidate's probe (phase 2 reads it from seq)
  float4 q_a[kKPW];                  // per owner, what the acceptance test needs of the query keyline: norm_t, sigma2_t, gradient
  float q_gn[kKPW];                  // ... and its norm
  int best[kKPW];                    // per owner: min over accepted candidates of slot << 16 | list position
  float w_f[7][kKPW];                // staged winner per owner: pos_img, (rho, sigma_rho), gradient, norm (rotated) ...
  int w_i[3][kKPW];                  // ... matches, match_id_keyframe, old keyline index
  float4 s_a[kBatch];                // probe geometry of the open keylines: t_x, t_y, pi0x, pi0y
  float4 s_b[kBatch];                // dq_min, dq_max, t_steps (int bits), -
  float seq[kBatch][2][kDmcWinPitch];  // [open keyline][0: tn, 1: tp][step - window start]
};
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// Exclusive prefix sum over the wave through the DPP data path (row_shr 1, 2, 4, 8 inside each row of 16 lanes, then row_bcast 15
// into rows 1 and 3 and row_bcast 31 into rows 2 and 3: twelve VALU instructions, no LDS crossbar); *total is a scalar.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_add_i(int v) {
  return v + __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xF, true);
}
__device__ __forceinline__ int wave_excl_scan_i(int v, int lane, int* total) {
  (void)lane;
  int incl = v;
  incl = dpp_add_i<0x111, 0xF>(incl);  // row_shr:1
  incl = dpp_add_i<0x112, 0xF>(incl);  // row_shr:2
  incl = dpp_add_i<0x114, 0xF>(incl);  // row_shr:4
  incl = dpp_add_i<0x118, 0xF>(incl);  // row_shr:8
  incl = dpp_add_i<0x142, 0xA>(incl);  // row_bcast:15 -> rows 1, 3
  incl = dpp_add_i<0x143, 0xC>(incl);  // row_bcast:31 -> rows 2, 3
  *total = __builtin_amdgcn_readlane(incl, 63);  // (a scalar: loops over the total are uniform)
  return incl - v;
}
// Acceptance test of one candidate (edge_map.cpp:170-177) on the two query scalars it needs of the probe geometry.
__device__ __forceinline__ bool search_accept_q(const KParams& p, float norm_t, float sigma2_t, float t, float2 cg, float cgn, float2 crs,
                                                float2 gq, float gnq) {
  SearchSetup S;
  S.norm_t = norm_t;
  S.sigma2_t = sigma2_t;
  return search_accept(p, S, t, cg, cgn, crs, gq, gnq);
}
// Test the T listed candidates of a wave, 64 at a time; accepted ones bid for their owner, the current best of an owner is staged.
template <bool kPhase2, class DmcWaveT>
__device__ __forceinline__ void dmc_test_list(const KParams& p, const MapDev& om, DmcWaveT& W, int T, int lane, int rot, const Mat3& R0,
                                              int step0) {
  for (int e0 = 0; e0 < T; e0 += 64) {
    const int e = e0 + lane;
    bool acc = false;
    OldKl ck{};
    int owner = 0, bid = 0, c = -1;
    if (e < T) {
      const unsigned ent = W.list[e];
      c = (int)(ent >> 16);
      owner = (int)((ent >> 10) & 63u);
      const int slot = (int)(ent & 1023u);
      const float t = kPhase2 ? W.seq[owner][slot & 1][(slot >> 1) - step0] : W.t1[e];
      ck = load_old(om, c, rot, R0, p.fm);
      const float4 qa = W.q_a[owner];
      acc = search_accept_q(p, qa.x, qa.y, t, ck.g, ck.gn, ck.rs, make_float2(qa.z, qa.w), W.q_gn[owner]);
      bid = (slot << 16) | e;
      if (acc) atomicMin(&W.best[owner], bid);
    }
    wave_lds_sync();
    if (acc && W.best[owner] == bid) {  // best so far of this owner (a later 64 may still replace it: same wave, program order)
      W.w_f[0][owner] = ck.pi.x; W.w_f[1][owner] = ck.pi.y; W.w_f[2][owner] = ck.rs.x; W.w_f[3][owner] = ck.rs.y;
      W.w_f[4][owner] = ck.g.x; W.w_f[5][owner] = ck.g.y; W.w_f[6][owner] = ck.gn;
      W.w_i[0][owner] = (int)ck.matches; W.w_i[1][owner] = ck.kf; W.w_i[2][owner] = c;
    }
    wave_lds_sync();
  }
}
template <class DmcWaveT>
__device__ __forceinline__ int dmc_commit(MapDev& nm, const MapDev& om, DmcWaveT& W, int owner, int idx, int* kf) {
  OldKl k;
  k.pi = make_float2(W.w_f[0][owner], W.w_f[1][owner]);
  k.rs = make_float2(W.w_f[2][owner], W.w_f[3][owner]);
  k.g = make_float2(W.w_f[4][owner], W.w_f[5][owner]);
  k.gn = W.w_f[6][owner];
  k.matches = (unsigned)W.w_i[0][owner];
  k.kf = W.w_i[1][owner];
  const int found = W.w_i[2][owner];
  search_commit(nm, om, idx, found, k, kf);
  return found;
}

template <int kThreads, int kLPK>
__device__ __forceinline__ void directed_match_c_body(KParams p, MapDev nm, MapDev om, Vec3 vel_, Mat3 Rvel_, Mat3 Rback_, float max_radius,
                                                      int rot_, Mat3 R0_, const GlueDev* __restrict__ gd, const GlueStage* __restrict__ stage) {
  static_assert(kLPK == 1 || kLPK == 2 || kLPK == 4 || kLPK == 8, "lanes per keyline");
  constexpr int kWaves = kThreads / 64;
  constexpr int kKPW = 64 / kLPK;                 // keylines per wave
  constexpr int kHP = 2 * kHeadSteps / kLPK;      // head probes per lane
  constexpr int kBatch = kKPW < kDmcOpen ? kKPW : kDmcOpen;
  static_assert(kMaxRecBlocks * 256 <= 65536, "old keyline index in 16 bits of a list entry");
  __shared__ DmcWave<kKPW, kBatch> lds[kWaves];
  const uint2 vb = xcd_band_block();
  if (p.dbg && vb.x == 0 && threadIdx.x == 0) p.dbg[48] = __builtin_amdgcn_s_memrealtime();
  const bool stats = p.dm_stats != nullptr;
  unsigned long long tk[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t_prev = stats ? __builtin_amdgcn_s_memrealtime() : 0ull;
#define RH_DMC_TICK(i)                                               \
  if (stats) {                                                       \
    const unsigned long long now_ = __builtin_amdgcn_s_memrealtime(); \
    tk[i] += now_ - t_prev;                                          \
    t_prev = now_;                                                   \
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int kl = lane / kLPK, sub = lane % kLPK;  // keyline of the wave, lane of the keyline
  DmcWave<kKPW, kBatch>& W = lds[wid];
  const int idx = (vb.x * kWaves + wid) * kKPW + kl;
  // bound-free early loads (arrays padded to the grid), issued before the parameter block is read
  const float2 pi = nm.pos_img[idx];
  const float2 rsq = nm.rs[idx];
  const float2 gq = nm.grad[idx];
  const float gnq = nm.gnorm[idx];
  const int n = nm.st->n;
  if (stage && vb.x == gridDim.x - 1 && wid == kWaves - 1) {
    // The pair's host record, left in device memory by the glue at the tail of the LM kernel (GlueStage): this wave - the last
    // of the grid, which owns no keyline unless the map is full - copies it into the pinned record while the launch works, waits
    // for its stores to be acknowledged and stamps the record and the pair's result slot (what the host compares, -12).
    const unsigned* src = reinterpret_cast<const unsigned*>(&stage->rec);
    GlueRec* hr = stage->host_rec;
    unsigned* dst = reinterpret_cast<unsigned*>(hr);
    constexpr int kWords = (int)(offsetof(GlueRec, seq_gs) / sizeof(unsigned));
    for (int i = lane; i < kWords; i += 64) dst[i] = src[i];
    const unsigned seq = stage->seq;
    PairSlot* hs = stage->host_slot;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): every lane's stores acknowledged (see stamp_drain)
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
      __hip_atomic_store(&hr->seq_gs, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(&hr->seq_out, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      if (hs) __hip_atomic_store(&hs->seq, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  const DmArgs A = dm_args(gd, vel_, Rvel_, Rback_, rot_, R0_);
  if (A.skip) return;
  const bool live = idx < n;
  SearchSetup S{};
  if (live) S = search_setup(p, pi, rsq, gq, gnq, A.vel, A.Rvel, A.Rback, max_radius);
  // ---- phase 1: the first kHeadSteps steps (edge_map.cpp:149-181). Slot 2 * step + side belongs to lane slot / kHP of the keyline;
  // every lane walks both chains through all kHeadSteps steps (8 adds) and keeps the values of its own slots.
  float tn = S.dq_rho, tp = S.dq_rho + 1.0f;
  float tq[kHP];
  int cand[kHP];
  {
    int prow[kHP], pcol[kHP];
#pragma unroll
    for (int h = 0; h < kHP; ++h) {
      prow[h] = -1;
      pcol[h] = 0;
      tq[h] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < kHeadSteps; ++j) {
      const bool active = live && j < S.t_steps;
#pragma unroll
      for (int i_idx = 0; i_idx < 2; ++i_idx) {
        const int slot = 2 * j + i_idx;
        const int h = slot % kHP;  // compile-time after unrolling
        if (slot / kHP == sub) {
          const float t = i_idx ? tp : tn;
          const bool ok = active && (i_idx ? !(t > S.dq_max) : !(t < S.dq_min));
          if (ok) {
            const int row = cvtt_f32(roundf(S.t_y * t + S.pi0y));
            const int col = cvtt_f32(roundf(S.t_x * t + S.pi0x));
            if ((unsigned)row < (unsigned)p.rows && (unsigned)col < (unsigned)p.cols) {
              prow[h] = row;
              pcol[h] = col;
            }
          }
          tq[h] = t;
        }
      }
      tp += 1.0f;
      tn -= 1.0f;
    }
#pragma unroll
    for (int h = 0; h < kHP; ++h) cand[h] = (prow[h] >= 0) ? om.mask[(size_t)prow[h] * p.cols + pcol[h]] : -1;
  }
  if (sub == 0) {
    W.best[kl] = kDmcNone;
    W.q_a[kl] = make_float4(S.norm_t, S.sigma2_t, gq.x, gq.y);
    W.q_gn[kl] = gnq;
  }
  int cnt = 0;
#pragma unroll
  for (int h = 0; h < kHP; ++h) cnt += (cand[h] >= 0) ? 1 : 0;
  RH_DMC_TICK(0)  // set-up, head probes issued
  int T = 0;
  int pos = wave_excl_scan_i(cnt, lane, &T);
  RH_DMC_TICK(1)  // mask loads back, scan
#pragma unroll
  for (int h = 0; h < kHP; ++h) {
    if (cand[h] >= 0) {
      W.list[pos] = ((unsigned)cand[h] << 16) | ((unsigned)kl << 10) | (unsigned)(sub * kHP + h);
      W.t1[pos] = tq[h];
      ++pos;
    }
  }
  wave_lds_sync();
  dmc_test_list<false>(p, om, W, T, lane, A.rot, A.R0, 0);
  int found = -1, kf = 0;
  if (sub == 0 && W.best[kl] != kDmcNone) found = dmc_commit(nm, om, W, kl, idx, &kf);
  RH_DMC_TICK(2)  // head candidates tested, commits issued
  // ---- phase 2: long searches still open (flagged on the first lane of the keyline)
  const bool open = live && sub == 0 && found < 0 && S.t_steps > kHeadSteps;
  const unsigned long long open_mask = __ballot(open);
  const int n_open = __popcll(open_mask);
  if (p.dbg && vb.x == 0 && threadIdx.x == 0) p.dbg[49] = __builtin_amdgcn_s_memrealtime();
  const int T_head = T;
  const int found_head = found;
  unsigned long long T2_sum = 0ull;
  // rank of this lane's keyline among the open ones (the same for all lanes of the keyline)
  const int rank = __popcll(open_mask & ((1ull << (kl * kLPK)) - 1ull));
  const bool kl_open = ((open_mask >> (kl * kLPK)) & 1ull) != 0ull;
  for (int b0 = 0; b0 < n_open; b0 += kBatch) {
    wave_lds_sync();  // (the previous batch's tables are still being read until here)
    const bool mine = kl_open && rank >= b0 && rank < b0 + kBatch;  // all lanes of the batch's keylines
    const int jj = rank - b0;
    const int nb = min(kBatch, n_open - b0);
    if (mine && sub == 0) {
      W.s_a[jj] = make_float4(S.t_x, S.t_y, S.pi0x, S.pi0y);
      W.s_b[jj] = make_float4(S.dq_min, S.dq_max, __int_as_float(S.t_steps), 0.f);
      W.q_a[jj] = make_float4(S.norm_t, S.sigma2_t, gq.x, gq.y);
      W.q_gn[jj] = gnq;
      W.best[jj] = kDmcNone;
    }
    // no search is longer than the radius allows: in search_setup dq_rho <= dq_max <= fl(max_radius + pu) and dq_min >= -pu (pu =
    // pixel_uncertainty_match), so t_steps = cvtt(fl(dq_rho - dq_min)) <= cvtt(fl(fl(max_radius + pu) + pu)) - rounding is
    // monotonic, so the same two additions give the bound itself and no slack is needed (the other branches are shorter: dq_max -
    // dq_rho <= dq_max, and the midpoint start probes only inside [dq_min, dq_max]). That is max_radius + 2 pu, not + pu: the
    // descending chain runs from dq_max down to -pu. Bounded at create and in rebvio_hip_directed_match, so a slot 2 * step + side
    // stays inside its 10 bits. With the defaults (40, 2) this is 44: the one window [kHeadSteps, kHeadSteps + kDmcWin)
    // (This holds for keylines of the domain: rho > 0 in front of the camera, p_m3[2] > 0, so dq_rho >= 0. An uploaded map with a
    // negative rho has dq_max - dq_rho > dq_max: its search is cut at this bound, while k_search_match_one walks all of it.)
    const int tmax = cvtt_f32((max_radius + p.pixel_uncertainty_match) + p.pixel_uncertainty_match);
    for (int step0 = kHeadSteps; step0 < tmax; step0 += kDmcWin) {
      // the chains continue through this window (tn, tp stand at step0): with two or more lanes per keyline lane 0 walks tn and
      // lane 1 tp (x - 1.0f and x + (-1.0f) are the same IEEE operation), a lone lane walks both
      const int wlen = min(kDmcWin, tmax - step0);
      // (always a whole window of kDmcWin steps, unrolled: one add and one LDS store with an immediate offset per step; what lies
      // beyond a keyline's t_steps is never read)
      if (kLPK >= 2) {
        if (mine && sub < 2) {
          float x = sub == 1 ? tp : tn;
          const float d = sub == 1 ? 1.0f : -1.0f;
          float* dst = &W.seq[jj][sub][0];
#pragma unroll
          for (int s = 0; s < kDmcWin; ++s) {
            dst[s] = x;
            x += d;
          }
          if (sub == 0) tn = x;
          else tp = x;
        }
      } else {
        if (mine) {  // (the owners of later batches keep their chains at step kHeadSteps)
#pragma unroll
          for (int s = 0; s < kDmcWin; ++s) {
            W.seq[jj][0][s] = tn;
            W.seq[jj][1][s] = tp;
            tp += 1.0f;
            tn -= 1.0f;
          }
        }
      }
      wave_lds_sync();
      RH_DMC_TICK(3)  // chains walked
      // probe slots of the batch, dealt to all 64 lanes: q -> (open keyline j, side, step); the first kDmcWin of a keyline's
      // 2 * kDmcWin slots walk tn, the others tp, so that neighbouring lanes probe neighbouring pixels of one line
      constexpr int kProbeIters = (kBatch * 2 * kDmcWin + 63) / 64;
      int pc[kProbeIters];
      unsigned pm[kProbeIters];
      constexpr int per = 2 * kDmcWin;
      const int nslots = nb * per;
      int pj = 0, ps = lane;  // slot of this lane in round 0: (open keyline, position); +64 slots per round
      unsigned pok = 0u;      // which of this lane's probes count
      // Rounds in chunks of kChunk behind ONE uniform test: inside a chunk nothing branches and no loaded value is looked at (a
      // select on it would make every round wait for its own load), so the LDS reads and mask loads of a chunk's rounds overlap.
      constexpr int kChunk = 5;
      static_assert(kProbeIters % kChunk == 0, "probe rounds per chunk");
#pragma unroll
      for (int c = 0; c < kProbeIters / kChunk; ++c) {
        if (c * kChunk * 64 < nslots) {  // (uniform)
#pragma unroll
          for (int u = 0; u < kChunk; ++u) {
            const int i = c * kChunk + u;
            const int j = min(pj, nb - 1);
            const int side = ps >= kDmcWin ? 1 : 0, so = ps - side * kDmcWin;
            const int step = step0 + so;
            const float4 sb = W.s_b[j];
            const float4 sa = W.s_a[j];
            const float t = W.seq[j][side][so];
            const int bj = W.best[j];
            bool ok = pj < nb && so < wlen && step < __float_as_int(sb.z) && bj == kDmcNone;
            ok = ok && (side ? !(t > sb.y) : !(t < sb.x));
            const int row = cvtt_f32(roundf(sa.y * t + sa.w));
            const int col = cvtt_f32(roundf(sa.x * t + sa.z));
            ok = ok && (unsigned)row < (unsigned)p.rows && (unsigned)col < (unsigned)p.cols;
            pc[i] = om.mask[ok ? row * p.cols + col : 0];
            pok |= ok ? (1u << i) : 0u;
            pm[i] = ((unsigned)j << 10) | (unsigned)(2 * step + side);
            ps += 64;  // (64 < per: at most one wrap)
            if (ps >= per) {
              ps -= per;
              ++pj;
            }
          }
        } else {
#pragma unroll
          for (int u = 0; u < kChunk; ++u) {
            pc[c * kChunk + u] = -1;
            pm[c * kChunk + u] = 0u;
          }
        }
      }
      RH_DMC_TICK(4)  // long-search probes issued
      int c2 = 0;
#pragma unroll
      for (int i = 0; i < kProbeIters; ++i) {
        if (!((pok >> i) & 1u)) pc[i] = -1;
        c2 += (pc[i] >= 0) ? 1 : 0;
      }
      int T2 = 0;
      int pos2 = wave_excl_scan_i(c2, lane, &T2);
      RH_DMC_TICK(5)  // mask loads back, scan
#pragma unroll
      for (int i = 0; i < kProbeIters; ++i) {
        if (pc[i] >= 0) {
          W.list[pos2] = ((unsigned)pc[i] << 16) | pm[i];
          ++pos2;
        }
      }
      wave_lds_sync();
      T2_sum += (unsigned long long)T2;
      dmc_test_list<true>(p, om, W, T2, lane, A.rot, A.R0, step0);
    }
    if (mine && sub == 0 && W.best[jj] != kDmcNone) found = dmc_commit(nm, om, W, jj, idx, &kf);
    RH_DMC_TICK(6)  // long-search candidates tested, commits issued
  }
  if (stats) {  // REBVIO_HIP_DM_STATS: one record per wave (plain stores; the host aggregates them in rebvio_hip_flush)
    const int c_live = __popcll(__ballot(live && sub == 0)), c_long = __popcll(__ballot(live && sub == 0 && S.t_steps > kHeadSteps));
    const int c_f1 = __popcll(__ballot(found_head >= 0));
    if (lane == 0) {
      unsigned long long* r = p.dm_stats + 16 * (size_t)(1 + vb.x * kWaves + wid);
#pragma unroll
      for (int i = 0; i < 7; ++i) r[i] = tk[i];
      r[8] = (unsigned long long)c_live; r[9] = (unsigned long long)c_long; r[10] = (unsigned long long)c_f1;
      r[11] = (unsigned long long)n_open; r[12] = (unsigned long long)T_head; r[13] = T2_sum;
      if (vb.x == 0 && wid == 0) p.dm_stats[0] = (unsigned long long)(gridDim.x * kWaves);
    }
  }
#undef RH_DMC_TICK
  // counters: wave -> workgroup (LDS) -> one global atomic per workgroup and counter (see k_directed_match)
  const int c_found = __popcll(__ballot(found >= 0));
  const int c_kf = __popcll(__ballot(kf != 0));
  if (kWaves == 1) {
    if (lane == 0) {
      if (c_found) atomicAdd(&nm.st->dm_matches, c_found);
      if (c_kf) atomicAdd(&nm.st->dm_kf, c_kf);
      if (n_open) atomicAdd(&nm.st->dm_queued, n_open);
    }
  } else {
    __shared__ int w_cnt[kWaves][3];
    if (lane == 0) {
      w_cnt[wid][0] = c_found;
      w_cnt[wid][1] = c_kf;
      w_cnt[wid][2] = n_open;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
      int t = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) t += w_cnt[w][threadIdx.x];
      int* dst = threadIdx.x == 0 ? &nm.st->dm_matches : (threadIdx.x == 1 ? &nm.st->dm_kf : &nm.st->dm_queued);
      if (t) atomicAdd(dst, t);
    }
  }
}

template <int kThreads, int kLPK>
__global__ __launch_bounds__(kThreads) void k_directed_match_c(KParams p, MapDev nm, MapDev om, Vec3 vel_, Mat3 Rvel_, Mat3 Rback_,
                                                               float max_radius, int rot_, Mat3 R0_, const GlueDev* __restrict__ gd,
                                                               const GlueStage* __restrict__ stage) {
  directed_match_c_body<kThreads, kLPK>(p, nm, om, vel_, Rvel_, Rback_, max_radius, rot_, R0_, gd, stage);
}
template <int kThreads, int kLPK>
__global__ __launch_bounds__(kThreads) void k_directed_match_c_b(KParams p, const LaneStatic* __restrict__ ls, const MapDev* __restrict__ maptab,
                                                                 LaneDynB dyn, float max_radius) {
  const LaneStatic& L = ls[blockIdx.z];
  const LaneDyn d = dyn.v[blockIdx.z];
  const Vec3 z3{};
  const Mat3 z9{};
  directed_match_c_body<kThreads, kLPK>(p, global_map(lane_map(maptab, blockIdx.z, d.nm, d.nm_swap)),
                                        global_map(lane_map(maptab, blockIdx.z, d.om, d.om_swap)), z3, z9, z9, max_radius, 1, z9,
                                        gptr(L.glue_dev) + d.slot, gptr(L.glue_stage) + d.slot);
}

// ---- EdgeMap::searchMatch as a public single-keyline call (edge_map.hpp:93-94, edge_map.cpp:101-184) ----------------
// One lane walks the reference's alternating probe sequence with the same set-up / acceptance code as the directedMatch
// kernels (vel / Rvel as given: directedMatch rotates them by Rback before it calls searchMatch, edge_map.cpp:193-194).
__global__ void k_search_match_one(KParams p, MapDev om, float2 pi, float2 rsq, float2 gq, float gnq, Vec3 vel, Mat3 Rvel,
                                   Mat3 Rback, float max_radius, int* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const SearchSetup S = search_setup(p, pi, rsq, gq, gnq, vel, Rvel, Rback, max_radius);
  Mat3 I{};
  int found = -1;
  float tn = S.dq_rho, tp = S.dq_rho + 1.0f;
  for (int t_i = 0; t_i < S.t_steps && found < 0; ++t_i, tp += 1.0f, tn -= 1.0f) {
    for (int i_idx = 0; i_idx < 2 && found < 0; ++i_idx) {
      const float t = i_idx ? tp : tn;
      if (i_idx ? (t > S.dq_max) : (t < S.dq_min)) continue;
      const int row = cvtt_f32(roundf(S.t_y * t + S.pi0y));
      const int col = cvtt_f32(roundf(S.t_x * t + S.pi0x));
      if ((unsigned)row >= (unsigned)p.rows || (unsigned)col >= (unsigned)p.cols) continue;
      const int cand = om.mask[(size_t)row * p.cols + col];
      if (cand < 0) continue;
      const OldKl ck = load_old(om, cand, 0, I, p.fm);
      if (search_accept(p, S, t, ck.g, ck.gn, ck.rs, gq, gnq)) found = cand;
    }
  }
  *out = found;
}

// ---- EdgeMap::regularize1Iter (edge_map.cpp:220-259): Jacobi step, results staged in rs_tmp ----------------------
__global__ __launch_bounds__(256) void k_regularize(KParams p, MapDev m, int gate_min_matches) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const float2 rs = m.rs[idx];  // bound-free early loads
  const int in = m.id_next[idx], ip = m.id_prev[idx];
  const int n = m.st->n;
  if (gate_min_matches > 0 && m.st->dm_matches < gate_min_matches) return;
  int set = 0;
  if (idx < n) {
    float2 out = rs;
    if (in >= 0 && ip >= 0) {
      const float2 rn = m.rs[in], rp = m.rs[ip];
      if (!((rn.x - rp.x) * (rn.x - rp.x) > (rn.y * rn.y + rp.y * rp.y))) {
        const float2 gn = m.grad[in], gp = m.grad[ip];
        float alpha = (gn.x * gp.x + gn.y * gp.y) / (m.gnorm[in] * m.gnorm[ip]);
        if (!(alpha < p.regularization_threshold)) {
          alpha = (float)((double)(alpha - p.regularization_threshold) / (1.0 - (double)p.regularization_threshold));
          alpha = (float)((double)alpha / ((double)(fabsf(rn.x - rp.x) / (rn.y + rp.y)) + 1.0));
          const float wr = (float)(1.0 / (double)(rs.y * rs.y));
          const float wrn = alpha / (rn.y * rn.y);
          const float wrp = alpha / (rp.y * rp.y);
          out.x = (rs.x * wr + rn.x * wrn + rp.x * wrp) / (wr + wrn + wrp);
          out.y = (rs.y * wr + rn.y * wrn + rp.y * wrp) / (wr + wrn + wrp);
          set = 1;
        }
      }
    }
    m.rs_tmp[idx] = out;
  }
  const int c = wave_sum_i(set);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&m.st->reg_count, c);
}

// ---- Core::updateInverseDepth[ARLU] (core.cpp:417-456): scalar EKF per matched keyline ----------------------------
__global__ __launch_bounds__(256) void k_depth_ekf(KParams p, MapDev m, Vec3 vel, int use_tmp, int gate_min_matches) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  float2 rs = use_tmp ? m.rs_tmp[idx] : m.rs[idx];  // bound-free early loads
  const int mid = m.match_id[idx];
  const float2 q = m.pos_img[idx];
  const float2 q0 = m.mpos_img[idx];
  const float2 mg = m.mgrad[idx];
  const float mgn = m.mgnorm[idx];
  const int n = m.st->n;
  if (gate_min_matches > 0 && m.st->dm_matches < gate_min_matches) return;
  if (idx >= n) return;
  if (mid >= 0) {
    const float vx = vel.a[0], vy = vel.a[1], vz = vel.a[2];
    float v_rho = rs.y * rs.y;
    const float ux = mg.x / mgn;
    const float uy = mg.y / mgn;
    const float Y = ux * (q.x - q0.x) + uy * (q.y - q0.y);
    const float H = ux * (vx * p.fm - vz * q0.x) + uy * (vy * p.fm - vz * q0.y);
    const float rho_p = (float)(1.0 / (1.0 / (double)rs.x + (double)vz));
    float F = (float)(1.0 / (1.0 + (double)(rs.x * vz)));
    F *= F;
    const float p_p = F * v_rho * F + p.reshape_q_abs * p.reshape_q_abs;
    const float e = Y - H * rho_p;
    const float S = H * p_p * H + p.pixel_uncertainty * p.pixel_uncertainty;
    const float K = (float)((double)(p_p * H) * (1.0 / (double)S));
    float rho = rho_p + K * e;
    v_rho = (float)((1.0 - (double)(K * H)) * (double)p_p);
    float sig = sqrtf(v_rho);
    if (rho < kRhoMin) {
      sig += kRhoMin - rho;
      rho = kRhoMin;
    } else if (rho > kRhoMax) {
      rho = kRhoMax;
    } else if (isnan(rho) || isnan(sig) || isinf(rho) || isinf(sig)) {
      rho = kRhoInit;
      sig = kRhoMax;
    }
    rs = make_float2(rho, sig);
  }
  m.rs[idx] = rs;
}

// ---- regularize1Iter + updateInverseDepth fused (edge_map.cpp:220-259, core.cpp:417-456) ------------------------
// Jacobi semantics need the neighbours' OLD depths: read rs, write rs_tmp; the host then swaps the two pointers of
// this map. Optionally (streaming driver) the keyline is also put through the NEXT pair's first rotateKeylines
// (rebvio.cpp:165) and binned for its estimateQuantile, which removes that pair's k_rotate launch.
// gd != null: vel / next rotation come from *gd; gd->nan_v (rebvio.cpp:236) leaves rho untouched like the match gate.
__device__ __forceinline__ void regularize_ekf_body(KParams p, MapDev m, Vec3 vel_, int gate_min_matches,
                                                        int next_rot_, Mat3 Rnext_,
                                                        int* __restrict__ hist, int hist_bins, const GlueDev* __restrict__ gd) {
  const uint2 vb = xcd_band_block();  // which keylines / tiles this workgroup takes: contiguous bands per XCD (common.hpp)
  __shared__ int sh[128];
  if (p.dbg && vb.x == 0 && threadIdx.x == 0) p.dbg[50] = __builtin_amdgcn_s_memrealtime();
  const int idx = vb.x * 256 + threadIdx.x;
  const float2 rs = m.rs[idx];  // bound-free early loads, issued before the parameter block is read
  const int in = m.id_next[idx], ip = m.id_prev[idx];
  const int mid = m.match_id[idx];
  float2 q = m.pos_img[idx];
  const float2 q0 = m.mpos_img[idx];
  const float2 mg = m.mgrad[idx];
  const float mgn = m.mgnorm[idx];
  float2 g = m.grad[idx];
  const int n = m.st->n;
  const int dm_matches = m.st->dm_matches;
  Vec3 vel = vel_;
  Mat3 Rnext = Rnext_;
  int next_rot = next_rot_;
  bool skip_pair = false;
  if (gd) {
#pragma unroll
    for (int i = 0; i < 3; ++i) vel.a[i] = gd->V[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) Rnext.a[i] = gd->RT_next[i];
    next_rot = gd->has_next;
    skip_pair = gd->nan_v != 0;
  }
  // both neighbours' depth, gradient and norm in ONE gather round trip (index 0 stands in where there is no neighbour pair;
  // the values are only used under the same conditions as before)
  const bool has_nb = idx < n && in >= 0 && ip >= 0;  // (rows past n hold no valid ids)
  const int in_s = has_nb ? in : 0, ip_s = has_nb ? ip : 0;
  const float2 rn = m.rs[in_s], rp = m.rs[ip_s];
  const float2 gn = m.grad[in_s], gp = m.grad[ip_s];
  const float gnn = m.gnorm[in_s], gnp = m.gnorm[ip_s];
  const bool gated = skip_pair || (gate_min_matches > 0 && dm_matches < gate_min_matches);
  if (next_rot) {
    if (threadIdx.x < 128) sh[threadIdx.x] = 0;
    __syncthreads();
  }
  int set = 0;
  if (idx < n) {
    float2 out = rs;
    if (!gated) {
      if (has_nb) {
        if (!((rn.x - rp.x) * (rn.x - rp.x) > (rn.y * rn.y + rp.y * rp.y))) {
          float alpha = (gn.x * gp.x + gn.y * gp.y) / (gnn * gnp);
          if (!(alpha < p.regularization_threshold)) {
            alpha = (float)((double)(alpha - p.regularization_threshold) / (1.0 - (double)p.regularization_threshold));
            alpha = (float)((double)alpha / ((double)(fabsf(rn.x - rp.x) / (rn.y + rp.y)) + 1.0));
            const float wr = (float)(1.0 / (double)(rs.y * rs.y));
            const float wrn = alpha / (rn.y * rn.y);
            const float wrp = alpha / (rp.y * rp.y);
            out.x = (rs.x * wr + rn.x * wrn + rp.x * wrp) / (wr + wrn + wrp);
            out.y = (rs.y * wr + rn.y * wrn + rp.y * wrp) / (wr + wrn + wrp);
            set = 1;
          }
        }
      }
      if (mid >= 0) {
        const float vx = vel.a[0], vy = vel.a[1], vz = vel.a[2];
        float v_rho = out.y * out.y;
        const float ux = mg.x / mgn;
        const float uy = mg.y / mgn;
        const float Y = ux * (q.x - q0.x) + uy * (q.y - q0.y);
        const float H = ux * (vx * p.fm - vz * q0.x) + uy * (vy * p.fm - vz * q0.y);
        const float rho_p = (float)(1.0 / (1.0 / (double)out.x + (double)vz));
        float F = (float)(1.0 / (1.0 + (double)(out.x * vz)));
        F *= F;
        const float p_p = F * v_rho * F + p.reshape_q_abs * p.reshape_q_abs;
        const float e = Y - H * rho_p;
        const float S = H * p_p * H + p.pixel_uncertainty * p.pixel_uncertainty;
        const float K = (float)((double)(p_p * H) * (1.0 / (double)S));
        float rho = rho_p + K * e;
        v_rho = (float)((1.0 - (double)(K * H)) * (double)p_p);
        float sig = sqrtf(v_rho);
        if (rho < kRhoMin) {
          sig += kRhoMin - rho;
          rho = kRhoMin;
        } else if (rho > kRhoMax) {
          rho = kRhoMax;
        } else if (isnan(rho) || isnan(sig) || isinf(rho) || isinf(sig)) {
          rho = kRhoInit;
          sig = kRhoMax;
        }
        out = make_float2(rho, sig);
      }
    }
    if (next_rot) {
      rotate_one(Rnext, p.fm, q, out, g);
      m.pos_img[idx] = q;
      m.grad_tmp[idx] = g;  // neighbours still read the un-rotated m.grad in this kernel: the caller swaps the pointers
      m.residual[idx] = 0.f;
      int i = cvtt_f32(hist_bins * (out.y - kRhoMin) / (kRhoMax - kRhoMin));
      i = (i > hist_bins - 1) ? (hist_bins - 1) : i;
      i = (i < 0) ? 0 : i;
      atomicAdd(&sh[i], 1);
    }
    m.rs_tmp[idx] = out;
  }
  // regularised-keyline count: one global atomic per workgroup (see k_directed_match)
  __shared__ int b_reg;
  if (threadIdx.x == 0) b_reg = 0;
  __syncthreads();
  const int c = wave_sum_i(set);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&b_reg, c);
  __syncthreads();
  if (threadIdx.x == 0 && b_reg) atomicAdd(&m.st->reg_count, b_reg);
  if (next_rot) {
    if ((int)threadIdx.x < hist_bins && sh[threadIdx.x]) atomicAdd(&hist[threadIdx.x], sh[threadIdx.x]);
  }
}

__global__ __launch_bounds__(256) void k_regularize_ekf(KParams p, MapDev m, Vec3 vel_, int gate_min_matches,
                                                        int next_rot_, Mat3 Rnext_,
                                                        int* __restrict__ hist, int hist_bins, const GlueDev* __restrict__ gd) {
  regularize_ekf_body(p, m, vel_, gate_min_matches, next_rot_, Rnext_, hist, hist_bins, gd);
}
__global__ __launch_bounds__(256) void k_regularize_ekf_b(KParams p, const LaneStatic* __restrict__ ls, const MapDev* __restrict__ maptab,
                                                          LaneDynB dyn, int gate_min_matches) {
  const LaneStatic& L = ls[blockIdx.z];
  const LaneDyn d = dyn.v[blockIdx.z];
  const Vec3 z3{};
  const Mat3 z9{};
  regularize_ekf_body(p, global_map(lane_map(maptab, blockIdx.z, d.nm, d.nm_swap)), z3, gate_min_matches, 0, z9, gptr(L.hist), p.quantile_num_bins,
                      gptr(L.glue_dev) + d.slot);
}

// ---- launchers ------------------------------------------------------------------------------------------------------
static Mat3 mat3(const float* r) {
  Mat3 m;
  for (int i = 0; i < 9; ++i) m.a[i] = r[i];
  return m;
}
static Vec3 vec3(const float* r) {
  Vec3 v;
  for (int i = 0; i < 3; ++i) v.a[i] = r ? r[i] : 0.f;
  return v;
}

void launch_rotate(hipStream_t s, const KParams& p, const MapDev& m, const float R[9], int* hist, int zero_dm) {
  RH_LAUNCH(k_rotate, dim3(div_up(p.kmax, 256)), dim3(256), 0, s, p, m, mat3(R), hist, p.quantile_num_bins, zero_dm);
}

void launch_quantile(hipStream_t s, const KParams& p, const MapDev& m, int* hist, float pct, int bins, float* out_dev) {
  (void)hipMemsetAsync(hist, 0, sizeof(int) * 128, s);
  RH_LAUNCH(k_sigma_hist, dim3(div_up(p.kmax, 256)), dim3(256), 0, s, m, hist, bins);
  RH_LAUNCH(k_quantile, dim3(1), dim3(64), 0, s, m, (const int*)hist, bins, pct, out_dev);
}

void launch_try_vel(hipStream_t s, const KParams& p, const MapDev& oldm, const MapDev& newm, int mode_lm, int call,
                    int last, LmState* st_in, LmState* st_out, const float* part_prev, float* part_out, const int* hist,
                    int frame_count) {
  RH_LAUNCH(k_try_vel, dim3(div_up(p.kmax, 256)), dim3(256), 0, s, p, oldm, newm, mode_lm, call, last,
                     (const LmState*)st_in, st_out, part_prev, part_out, hist, (unsigned)frame_count);
}

// Speculative form (k_lm_chain_spec; do_ext == 2 / spec != 0 allows it, the context's REBVIO_HIP_LM=seq does not). Needs at
// least two speculative evaluations, at most kSpecMax, and the staged record sets in the default 64 KB of LDS with the static part.
// The LDS bound also keeps it to maps of up to ~40k keylines: with the attribute raised it ran at 64k keylines (1280x960,
// 125 workgroups) and was slower than the sequential kernel there (5.3k vs 6.5k frames/s) - four evaluations' arithmetic
// per pass on every workgroup and a 125-hop neighbour chain outweigh the three exchange rounds saved.
static size_t lm_spec_shm(int kmax, int calls) {
  const int groups = std::min(div_up(kmax, 256), kMaxRecBlocks);
  return (size_t)(calls - 2) * groups * kPartStride * sizeof(float);
}
static bool lm_spec_usable(int kmax, int calls, int kf = 2) {
  return calls - kf >= 2 && calls - 2 <= kSpecMax && calls <= kMaxLmCalls && lm_spec_shm(kmax, calls) <= 40 * 1024;
}

void launch_lm_chain(hipStream_t s, const KParams& p, const MapDev& oldm, const MapDev& newm, int calls, int do_ext, LmState* st_in,
                     LmState* st_out, unsigned long long* xch, unsigned tag_base, int* bar_err, const int* hist, float* xrv_part,
                     PairSlot* slot, int* hist_to_zero, unsigned long long* stamps, int threads, const GlueArgs& ga) {
  const dim3 grid((p.kmax + threads - 1) / threads);
  // do_ext: 1 = k_lm_chain; 2 / 3 = the speculative kernel with its first speculative evaluation at index 2 / 3 (lm_chain_spec_body)
  if (do_ext >= 2 && threads <= 512 && lm_spec_usable(p.kmax, calls, do_ext)) {
    const int kf = do_ext;
    if (threads == 256)
      RH_LAUNCH(k_lm_chain_spec<256>, grid, dim3(256), lm_spec_shm(p.kmax, calls), s, p, oldm, newm, calls, (const LmState*)st_in, st_out,
                xch, tag_base, bar_err, hist, xrv_part, slot, hist_to_zero, stamps, ga, kf);
    else
      RH_LAUNCH(k_lm_chain_spec<512>, grid, dim3(512), lm_spec_shm(p.kmax, calls), s, p, oldm, newm, calls, (const LmState*)st_in, st_out,
                xch, tag_base, bar_err, hist, xrv_part, slot, hist_to_zero, stamps, ga, kf);
    return;
  }
  if (do_ext >= 2) do_ext = 2;  // (k_lm_chain reads do_ext as "with forwardMatch / extRotVel")
  switch (threads) {
    case 256:
      RH_LAUNCH(k_lm_chain<256>, grid, dim3(256), 0, s, p, oldm, newm, calls, do_ext, (const LmState*)st_in, st_out, xch, tag_base,
                bar_err, hist, 0u, xrv_part, slot, hist_to_zero, stamps, ga);
      break;
    case 512:
      RH_LAUNCH(k_lm_chain<512>, grid, dim3(512), 0, s, p, oldm, newm, calls, do_ext, (const LmState*)st_in, st_out, xch, tag_base,
                bar_err, hist, 0u, xrv_part, slot, hist_to_zero, stamps, ga);
      break;
    default:
      RH_LAUNCH(k_lm_chain<1024>, grid, dim3(1024), 0, s, p, oldm, newm, calls, do_ext, (const LmState*)st_in, st_out, xch, tag_base,
                bar_err, hist, 0u, xrv_part, slot, hist_to_zero, stamps, ga);
  }
}

void launch_lm_final(hipStream_t s, const MapDev& oldm, int calls, LmState* st_in, LmState* st_out, const float* part_prev) {
  RH_LAUNCH(k_lm_final, dim3(1), dim3(256), 0, s, oldm, calls, (const LmState*)st_in, st_out, part_prev);
}

void launch_forward_keys(hipStream_t s, const KParams& p, const MapDev& oldm, const MapDev& newm) {
  RH_LAUNCH(k_forward_keys, dim3(div_up(p.kmax, 256)), dim3(256), 0, s, oldm, newm);
}

void launch_ext_rot_vel(hipStream_t s, const KParams& p, const MapDev& oldm, const MapDev& newm, int do_forward,
                        int do_lm_final, int calls, LmState* st_in, LmState* st_out, const float* part_prev,
                        float* xrv_part, const float* vel_manual, PairSlot* slot, int* hist_to_zero, unsigned seq) {
  RH_LAUNCH(k_ext_rot_vel, dim3(div_up(p.kmax, 256)), dim3(256), 0, s, p, oldm, newm, do_forward, do_lm_final,
                     calls, (const LmState*)st_in, st_out, part_prev, xrv_part, vec3(vel_manual), slot, hist_to_zero, seq);
}


// Form of the directedMatch launch, k_directed_match_c<threads, lanes per keyline> (REBVIO_HIP_DM_HEAD / REBVIO_HIP_BATCH_DM_HEAD, read
// at create; 0 = chosen here): 1 "compact8" <512, 8>, 2 "compact4" <256, 4>, 3 "compact1" <64, 1>.
// One stream of up to 32 768 keylines takes <512, 8>: eight keylines per wave, 1 875 short waves on an idle chip (MI355X, 640x480 /
// 15 k keylines: 15.6 k frames/s against 15.2 k for <256, 4>, 12.1 k for <64, 1>, 13.7 k for the two-launch form of round 3).
// Larger maps and batches of four lanes or more, where the chip is full, take the form with the fewest instructions, <64, 1>
// (1280x960 / 57 k keylines: 7.07 k frames/s against 6.26 k for <256, 4> and 6.69 k for round 3's form).
static int dm_form(int kmax, int head_form, int lanes) {
  if (head_form >= 1 && head_form <= 3) return head_form;
  return (kmax <= 32768 && lanes < 4) ? 1 : 3;
}
#define RH_DMC_DISPATCH(KERNEL, form, kmax, zdim, stream, ...)                                                                                 \
  do {                                                                                                                                         \
    switch (form) {                                                                                                                            \
      case 1: RH_LAUNCH_NAMED(#KERNEL "<512,8>", (KERNEL<512, 8>), dim3(div_up(kmax, 64), 1, zdim), dim3(512), 0, stream, __VA_ARGS__); break; \
      case 2: RH_LAUNCH_NAMED(#KERNEL "<256,4>", (KERNEL<256, 4>), dim3(div_up(kmax, 64), 1, zdim), dim3(256), 0, stream, __VA_ARGS__); break; \
      default: RH_LAUNCH_NAMED(#KERNEL "<64,1>", (KERNEL<64, 1>), dim3(div_up(kmax, 64), 1, zdim), dim3(64), 0, stream, __VA_ARGS__); break;   \
    }                                                                                                                                          \
  } while (0)

void launch_directed_match(hipStream_t s, const KParams& p, const MapDev& newm, const MapDev& oldm, const float vel[3],
                           const float Rvel[9], const float Rback[9], float max_radius, const float* R0_on_the_fly, int head_form) {
  const int form = dm_form(p.kmax, head_form, 1);
  const int rot = R0_on_the_fly ? 1 : 0;
  const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  const Mat3 R0 = mat3(R0_on_the_fly ? R0_on_the_fly : I);
  RH_DMC_DISPATCH(k_directed_match_c, form, p.kmax, 1, s, p, newm, oldm, vec3(vel), mat3(Rvel), mat3(Rback), max_radius, rot, R0,
                  (const GlueDev*)nullptr, (const GlueStage*)nullptr);
}

// the same launch with the second half's inputs read from *gd at run time: the record the pair's LM kernel left (device glue,
// glue_dev.hpp)
void launch_directed_match_dev(hipStream_t s, const KParams& p, const MapDev& newm, const MapDev& oldm, const GlueDev* gd,
                               const GlueStage* stage, float max_radius, int head_form) {
  const int form = dm_form(p.kmax, head_form, 1);
  const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, z[3] = {0, 0, 0};
  RH_DMC_DISPATCH(k_directed_match_c, form, p.kmax, 1, s, p, newm, oldm, vec3(z), mat3(I), mat3(I), max_radius, 1, mat3(I), gd, stage);
}

void launch_search_match_one(hipStream_t s, const KParams& p, const MapDev& searched, const rebvio_hip_keyline& q, const float vel[3],
                             const float Rvel[9], const float Rback[9], float max_radius, int* out_dev) {
  RH_LAUNCH(k_search_match_one, dim3(1), dim3(64), 0, s, p, searched, make_float2(q.pos_img[0], q.pos_img[1]),
            make_float2(q.rho, q.sigma_rho), make_float2(q.gradient[0], q.gradient[1]), q.gradient_norm, vec3(vel), mat3(Rvel),
            mat3(Rback), max_radius, out_dev);
}

void launch_regularize(hipStream_t s, const KParams& p, const MapDev& m, int gate) {
  RH_LAUNCH(k_regularize, dim3(div_up(p.kmax, 256)), dim3(256), 0, s, p, m, gate);
}

void launch_regularize_ekf(hipStream_t s, const KParams& p, const MapDev& m, const float vel[3], int gate, const float* Rnext, int* hist) {
  const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  RH_LAUNCH(k_regularize_ekf, dim3(div_up(p.kmax, 256)), dim3(256), 0, s, p, m, vec3(vel), gate, Rnext ? 1 : 0,
            mat3(Rnext ? Rnext : I), hist, p.quantile_num_bins, (const GlueDev*)nullptr);
}

void launch_regularize_ekf_dev(hipStream_t s, const KParams& p, const MapDev& m, const GlueDev* g_dev, int gate, int* hist) {
  const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, z[3] = {0, 0, 0};
  RH_LAUNCH(k_regularize_ekf, dim3(div_up(p.kmax, 256)), dim3(256), 0, s, p, m, vec3(z), gate, 0, mat3(I), hist,
                 p.quantile_num_bins, g_dev);
}

void launch_lm_chain_b(hipStream_t s, const KParams& p, int lanes, int lanes_per_launch, const LaneStatic* ls, const MapDev* maptab,
                       const LaneDynB& dyn, int calls, int spec, const GlueParams& gp, const LaneGyroB& gyro) {
  // 512-thread workgroups (the single-stream default). The workgroups of a lane wait for each other's records, and HIP promises
  // nothing about the order in which a grid's workgroups become resident (MI355X_MICROARCH.md, contract [G]): a launch carries
  // only as many lanes as fit the device TOGETHER (lm_chain_b_max_lanes: 8 lanes of 16 k keylines at one workgroup per CU), a
  // wider batch takes several launches back to back.
  const int slow_poll = lanes >= 3 ? 1 : 0;
  const int per = std::max(1, std::min(lanes, lanes_per_launch));
  const bool use_spec = spec >= 2 && lm_spec_usable(p.kmax, calls, spec);  // spec: 0 / 1 = k_lm_chain_b, 2 / 3 = first speculative evaluation
  for (int l0 = 0; l0 < lanes; l0 += per) {
    const dim3 grid((p.kmax + 511) / 512, 1, (unsigned)std::min(per, lanes - l0));
    if (use_spec)
      RH_LAUNCH(k_lm_chain_spec_b<512>, grid, dim3(512), lm_spec_shm(p.kmax, calls), s, p, ls, maptab, dyn, calls, slow_poll, gp, gyro, l0, spec);
    else
      RH_LAUNCH(k_lm_chain_b<512>, grid, dim3(512), 0, s, p, ls, maptab, dyn, calls, slow_poll, gp, gyro, l0);
  }
}

// How many lanes' workgroups of the batched persistent LM kernel the device holds at once: all workgroups of a launch poll
// their lane's records, so all of them have to be resident together whatever order they are dispatched in. One block per CU is
// taken off the occupancy query's answer where it admits several (MI355X_MICROARCH.md: the query can read one block per CU
// high); kernels of the other streams only delay residency, they do not depend on this one. 0: not even one lane fits.
int lm_chain_b_capacity_wgs(int device, int kmax, int calls) {
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) return 0;
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_lm_chain_b<512>, 512, 0) != hipSuccess) nb = 1;
  if (lm_spec_usable(kmax, calls)) {
    int nbs = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nbs, k_lm_chain_spec_b<512>, 512, lm_spec_shm(kmax, calls)) != hipSuccess) nbs = 1;
    nb = std::min(nb, nbs);
  }
  nb = nb > 1 ? nb - 1 : 1;
  return nb * cus;
}
int lm_chain_b_max_lanes(int device, int kmax, int calls) {
  const int cap = lm_chain_b_capacity_wgs(device, kmax, calls);
  if (cap <= 0) return 1;
  const int per_lane = (kmax + 511) / 512;
  return std::min(kMaxLanes, cap / per_lane);
}

// second half of a batched step (every lane's inputs come from the record its LM kernel's glue left)
void launch_b_chain_b(hipStream_t s, const KParams& p, int lanes, const LaneStatic* ls, const MapDev* maptab, const LaneDynB& dyn,
                      float max_radius, int gate, int head_form) {
  const unsigned z = (unsigned)lanes;
  const int form = dm_form(p.kmax, head_form, lanes);
  RH_DMC_DISPATCH(k_directed_match_c_b, form, p.kmax, z, s, p, ls, maptab, dyn, max_radius);
  RH_LAUNCH(k_regularize_ekf_b, dim3(div_up(p.kmax, 256), 1, z), dim3(256), 0, s, p, ls, maptab, dyn, gate);
}

void launch_depth_ekf(hipStream_t s, const KParams& p, const MapDev& m, const float vel[3], int use_tmp, int gate) {
  RH_LAUNCH(k_depth_ekf, dim3(div_up(p.kmax, 256)), dim3(256), 0, s, p, m, vec3(vel), use_tmp, gate);
}

// ---- point cloud of a map's depth-bearing keylines (rebvio_hip_map_point_cloud*; no reference counterpart) ------------------
// An order-preserving stream compaction over the keyline arrays in two launches of one workgroup per 256 keylines:
//   k_cloud_count  each workgroup's number of passing keylines -> blk_cnt[workgroup]
//   k_cloud_emit   block offset = sum of the counts in front of it (fixed order: integer sums), place within the block from a
//                  wave64 ballot + lane-prefix popcount and the wave totals in LDS; one 32-byte record = two 16-byte stores.
// A point's place depends on the keyline index alone - no atomic decides an order - so the cloud is reproducible bit for bit.
// Both write device memory. k_cloud_copy, on a stream of its own behind them, moves exactly the records that exist into
// host-visible memory: 16 bytes per lane, consecutive lanes consecutive addresses, so that the writes cross the bus as whole
// lines (records stored there by k_cloud_emit directly - 16 bytes per lane at a 32-byte stride, one bus write each - took 1.0 ms
// for 13 500 points). The count and the sequence stamp behind it are stored by the workgroup that finishes last (a
// ticket counter tells which: it orders nothing but that one store), after every workgroup's stores have left.
__device__ __forceinline__ bool cloud_pass(const CloudArgs& a, float2 rs, unsigned matches) {
  // positive tests: a NaN in rho or sigma_rho fails them
  return matches >= a.min_matches && rs.x >= a.rho_min && rs.x <= a.rho_max && rs.y <= a.max_rel_sigma * rs.x;
}
// (count of passing lanes in front of this lane, count of the wave)
__device__ __forceinline__ int2 wave_place(bool pass) {
  const unsigned long long b = __ballot(pass);
  const int before = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
  return make_int2(before, __popcll(b));
}

__global__ __launch_bounds__(256) void k_cloud_count(MapDev m, CloudArgs a, int* __restrict__ blk_cnt) {
  __shared__ int sh[4];
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const float2 rs = m.rs[idx];  // bound-free early loads (the arrays are padded to the launch grid)
  const unsigned mt = m.matches[idx];
  const int n = m.st->n;
  const int2 w = wave_place(idx < n && cloud_pass(a, rs, mt));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = w.y;
  __syncthreads();
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(256) void k_cloud_emit(KParams p, MapDev m, CloudArgs a, const int* __restrict__ blk_cnt,
                                                    int* __restrict__ count_out, float4* __restrict__ out) {
  __shared__ int sh_w[4], sh_lo[4], sh_all[4];
  const int tid = threadIdx.x, idx = blockIdx.x * 256 + tid, wv = tid >> 6;
  const float2 pi = m.pos_img[idx];
  const float2 rs = m.rs[idx];
  const float gn = m.gnorm[idx];
  const unsigned mt = m.matches[idx];
  const int n = m.st->n;
  // every workgroup's count, one per thread (gridDim.x <= kMaxRecBlocks = 256)
  const int c = tid < (int)gridDim.x ? blk_cnt[tid] : 0;
  const int lo = wave_sum_i(tid < (int)blockIdx.x ? c : 0), all = wave_sum_i(c);
  const bool pass = idx < n && cloud_pass(a, rs, mt);
  const int2 w = wave_place(pass);
  if ((tid & 63) == 0) {
    sh_w[wv] = w.y;
    sh_lo[wv] = lo;
    sh_all[wv] = all;
  }
  __syncthreads();
  int rank = (sh_lo[0] + sh_lo[1]) + (sh_lo[2] + sh_lo[3]) + w.x;
  for (int k = 0; k < wv; ++k) rank += sh_w[k];
  if (blockIdx.x == 0 && tid == 0) *count_out = (sh_all[0] + sh_all[1]) + (sh_all[2] + sh_all[3]);
  if (pass && rank < a.cap) {
    const float u = pi.x / p.fm, v = pi.y / p.fm;  // (the divisions of rotateKeylines, edge_map.cpp:60)
    const float z = a.scale / rs.x;
    const float xc = u * z, yc = v * z;
    float q[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) q[i] = ((a.R[3 * i] * xc + a.R[3 * i + 1] * yc) + a.R[3 * i + 2] * z) + a.t[i];
    // two 16-byte stores per record (volatile: left alone, the compiler re-cuts the 32 bytes into 12 + 12 + 8)
    typedef float v4f __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(1))) volatile v4f* GRec;  // (global_store, not flat_store: common.hpp gptr)
    GRec rec = (GRec)(out + 2 * (size_t)rank);
    rec[0] = v4f{q[0], q[1], q[2], rs.x};
    rec[1] = v4f{rs.y, gn, __int_as_float(idx), __uint_as_float(mt)};
  }
}

// records[0 .. min(*count, cap)) -> host-visible memory, then the head: count, and the stamp behind everything
__global__ __launch_bounds__(256) void k_cloud_copy(const float4* __restrict__ src, const int* __restrict__ count, int cap, unsigned seq,
                                                    unsigned* __restrict__ ticket, CloudHdr* __restrict__ hdr, float4* __restrict__ dst) {
  __shared__ int sh_last;
  const int total = *count;
  const int chunks = 2 * (total < cap ? total : cap);  // 16-byte pieces
  for (int i = blockIdx.x * 256 + threadIdx.x; i < chunks; i += gridDim.x * 256) dst[i] = src[i];
  // this wave's stores have left (host-visible memory is written through), then the workgroup takes its ticket
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) sh_last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u;
  __syncthreads();
  if (sh_last && threadIdx.x == 0) {
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // for the next copy (stream-ordered)
    hdr->count = total;
    stamp_drain(&hdr->seq, seq);
  }
}

void launch_point_cloud(hipStream_t s, const KParams& p, const MapDev& m, const CloudArgs& a, int* blk_cnt, int* count_dev,
                        void* records_dev) {
  const dim3 grid(div_up(p.kmax, 256));
  RH_LAUNCH(k_cloud_count, grid, dim3(256), 0, s, m, a, blk_cnt);
  RH_LAUNCH(k_cloud_emit, grid, dim3(256), 0, s, p, m, a, (const int*)blk_cnt, count_dev, reinterpret_cast<float4*>(records_dev));
}

void launch_point_cloud_copy(hipStream_t s, const KParams& p, const void* records_dev, const int* count_dev, const CloudArgs& a,
                             unsigned* ticket, CloudHdr* hdr, void* records_host) {
  const int blocks = std::max(1, std::min(64, div_up(2 * a.cap, 256)));
  RH_LAUNCH(k_cloud_copy, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const float4*>(records_dev), count_dev, a.cap, a.seq, ticket, hdr,
            reinterpret_cast<float4*>(records_host));
}

// ---- keyframes (rebvio_hip_map_mark_keyframe, rebvio_hip_keyframe_next, rebvio_hip_map_keyframe_matches) ------------------------
// match_id_keyframe (types/keyline.hpp:39) rides through forwardMatch and directedMatch (edge_map.cpp:93,210); the reference never
// sets it. k_mark_keyframe starts it: every keyline of the map becomes its own keyframe id. One coalesced dword store per lane;
// nothing else of the map is written.
__global__ __launch_bounds__(256) void k_mark_keyframe(MapDev m) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < m.st->n) m.match_kf[idx] = idx;
}

void launch_mark_keyframe(hipStream_t s, const KParams& p, const MapDev& m) {
  RH_LAUNCH(k_mark_keyframe, dim3(div_up(p.kmax, 256)), dim3(256), 0, s, m);
}

// Keyframe-to-current correspondences: per keyframe slot j < kf_size the keylines i of this map with match_id_keyframe[i] == j
// ("claimants"), their number, and the one of smallest sigma_rho (smallest index among equals) as the winner.
//   k_kf_claim  one thread per keyline: 64-bit atomicMin of (sigma key << 32 | i) and an integer atomicAdd into its slot - both
//               independent of the order the claims arrive in, so the table is the same bit for bit on every run
//   k_kf_count / k_kf_emit  the order-preserving compaction of k_cloud_count / k_cloud_emit over the slots that have a claimant
// The table (keys all-ones, counts zero) is initialised on the same stream in front of k_kf_claim (launch_kf_matches).
__device__ __forceinline__ unsigned kf_sigma_key(float sigma_rho) {
  // positive test: NaN and negative values sort behind everything (+inf included); + 0.0f folds -0.0 into +0.0
  return sigma_rho >= 0.0f ? __float_as_uint(sigma_rho + 0.0f) : 0xFFFFFFFFu;
}

__global__ __launch_bounds__(256) void k_kf_claim(MapDev m, int kf_size, unsigned long long* __restrict__ key, int* __restrict__ claimants) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int id = m.match_kf[idx];  // bound-free early loads (the arrays are padded to the launch grid)
  const float2 rs = m.rs[idx];
  if (idx >= m.st->n || id < 0 || id >= kf_size) return;
  atomicMin(key + id, ((unsigned long long)kf_sigma_key(rs.y) << 32) | (unsigned)idx);
  atomicAdd(claimants + id, 1);
}

__global__ __launch_bounds__(256) void k_kf_count(int kf_size, const int* __restrict__ claimants, int* __restrict__ blk_cnt) {
  __shared__ int sh[4];
  const int j = blockIdx.x * 256 + threadIdx.x;
  const int2 w = wave_place(j < kf_size && claimants[j] > 0);  // (the table covers the launch grid)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = w.y;
  __syncthreads();
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(256) void k_kf_emit(MapDev m, int kf_size, int cap, const unsigned long long* __restrict__ key,
                                                 const int* __restrict__ claimants, const int* __restrict__ blk_cnt,
                                                 int* __restrict__ count_out, float4* __restrict__ out) {
  __shared__ int sh_w[4], sh_lo[4], sh_all[4];
  const int tid = threadIdx.x, j = blockIdx.x * 256 + tid, wv = tid >> 6;
  const int cl = claimants[j];
  const unsigned long long k = key[j];
  // every workgroup's count, one per thread (gridDim.x <= kMaxRecBlocks = 256)
  const int c = tid < (int)gridDim.x ? blk_cnt[tid] : 0;
  const int lo = wave_sum_i(tid < (int)blockIdx.x ? c : 0), all = wave_sum_i(c);
  const bool pass = j < kf_size && cl > 0;
  const int2 w = wave_place(pass);
  if ((tid & 63) == 0) {
    sh_w[wv] = w.y;
    sh_lo[wv] = lo;
    sh_all[wv] = all;
  }
  __syncthreads();
  int rank = (sh_lo[0] + sh_lo[1]) + (sh_lo[2] + sh_lo[3]) + w.x;
  for (int i = 0; i < wv; ++i) rank += sh_w[i];
  if (blockIdx.x == 0 && tid == 0) *count_out = (sh_all[0] + sh_all[1]) + (sh_all[2] + sh_all[3]);
  if (pass && rank < cap) {
    const int win = (int)(unsigned)k;  // a claimant's index is below the map's size: k_kf_claim
    const float2 rs = m.rs[win];
    const float2 pi = m.pos_img[win];
    const unsigned mt = m.matches[win];
    // two 16-byte stores per record, as k_cloud_emit
    typedef float v4f __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(1))) volatile v4f* GRec;
    GRec rec = (GRec)(out + 2 * (size_t)rank);
    rec[0] = v4f{__int_as_float(j), __int_as_float(win), __int_as_float(cl), __uint_as_float(mt)};
    rec[1] = v4f{rs.x, rs.y, pi.x, pi.y};
  }
}

int launch_kf_matches(hipStream_t s, const KParams& p, const MapDev& m, int kf_size, int cap, unsigned long long* key, int* claimants,
                      int* blk_cnt, int* count_dev, void* records_dev) {
  // on THIS stream: a null-stream memset is not ordered against the context's non-blocking streams (alloc_map)
  const size_t slots = (size_t)div_up(p.kmax, 256) * 256;
  hipError_t e = hipMemsetAsync(key, 0xFF, slots * sizeof(unsigned long long), s);
  if (e == hipSuccess) e = hipMemsetAsync(claimants, 0, slots * sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  RH_LAUNCH(k_kf_claim, dim3(div_up(p.kmax, 256)), dim3(256), 0, s, m, kf_size, key, claimants);
  const dim3 grid(div_up(kf_size, 256));
  RH_LAUNCH(k_kf_count, grid, dim3(256), 0, s, kf_size, (const int*)claimants, blk_cnt);
  RH_LAUNCH(k_kf_emit, grid, dim3(256), 0, s, m, kf_size, cap, (const unsigned long long*)key, (const int*)claimants, (const int*)blk_cnt,
            count_dev, reinterpret_cast<float4*>(records_dev));
  return 0;
}

// ---- keyframe snapshot and keyframe-to-current pose (rebvio_hip_map_keyframe_snapshot, rebvio_hip_map_keyframe_pose) ------------
// k_kf_snapshot keeps what the pose needs of a keyframe in the keyframe's own frame: (pos_img, rho, sigma_rho) as one 16-byte
// record per keyline - one 16-byte store per lane - matches as a dword array, and the size. One workgroup per 256 keylines, the
// size read on the device; only the map's own n records are written.
__global__ __launch_bounds__(256) void k_kf_snapshot(MapDev m, float4* __restrict__ prs, unsigned* __restrict__ matches, int* __restrict__ n_out) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const float2 pi = m.pos_img[idx];  // bound-free early loads (the arrays are padded to the launch grid)
  const float2 rs = m.rs[idx];
  const unsigned mt = m.matches[idx];
  const int n = m.st->n;
  if (idx == 0) *n_out = n;
  if (idx < n) {
    prs[idx] = make_float4(pi.x, pi.y, rs.x, rs.y);
    matches[idx] = mt;
  }
}

void launch_kf_snapshot(hipStream_t s, const KParams& p, const MapDev& m, void* prs, unsigned* matches, int* n_out) {
  RH_LAUNCH(k_kf_snapshot, dim3(div_up(p.kmax, 256)), dim3(256), 0, s, m, reinterpret_cast<float4*>(prs), matches, n_out);
}

// What the keyframe solvers' kernels share (each inlined into its kernel).
// the pose of a result block in registers
__device__ __forceinline__ void kf_load_pose(const rebvio_hip_kf_pose* __restrict__ st, double* R, double* t) {
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = st->R[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = st->t[k];
}
// the field, pos and unit of a map as kfp::lookup reads them
__device__ __forceinline__ kfp::AlignMap kf_align_map(const KParams& p, const MapDev& m) {
  kfp::AlignMap c;
  c.fm = p.fm; c.cx = p.cx; c.cy = p.cy; c.rows = p.rows; c.cols = p.cols;
  c.df = m.df; c.df_nr = p.df_nr; c.ids = nullptr; c.dists = nullptr;
  c.pos = reinterpret_cast<const kfp::AlignF2*>(m.pos); c.unit = reinterpret_cast<const kfp::AlignF2*>(m.unit);
  c.cap = p.kmax;
  return c;
}
// The 28 addends of every lane of a workgroup of 256 reduced by a FIXED tree: an fp64 butterfly over the wave (every lane ends
// with the same total: a + b == b + a), the four wave totals through LDS as (w0 + w1) + (w2 + w3) -> part[blockIdx.x]; the lanes
// with `used` counted by ballot the same way -> part_used[blockIdx.x]. No floating-point atomic anywhere, so the sums are the same
// bit for bit on every run. kInl: the lanes with `inl` are counted as well, through sh_inl into part_inl (unused without it). sh:
// 4 x 28 doubles, sh_used / sh_inl: 4 ints of LDS each.
template <bool kInl>
__device__ __forceinline__ void kf_block_sums(double* v, bool used, bool inl, double (*sh)[kfp::kSums], int* sh_used, int* sh_inl,
                                              double* __restrict__ part, int* __restrict__ part_used, int* __restrict__ part_inl) {
  const int tid = threadIdx.x, wv = tid >> 6;
#pragma unroll
  for (int k = 0; k < kfp::kSums; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] = v[k] + __shfl_xor(v[k], o);
  }
  const int nu = __popcll(__ballot(used)), ni = kInl ? __popcll(__ballot(inl)) : 0;
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < kfp::kSums; ++k) sh[wv][k] = v[k];
    sh_used[wv] = nu;
    if (kInl) sh_inl[wv] = ni;
  }
  __syncthreads();
  if (tid < kfp::kSums) part[(size_t)blockIdx.x * kfp::kSums + tid] = (sh[0][tid] + sh[1][tid]) + (sh[2][tid] + sh[3][tid]);
  if (tid == 0) {
    part_used[blockIdx.x] = (sh_used[0] + sh_used[1]) + (sh_used[2] + sh_used[3]);
    if (kInl) part_inl[blockIdx.x] = (sh_inl[0] + sh_inl[1]) + (sh_inl[2] + sh_inl[3]);
  }
}
// sum k = tid < 28 of the first nb partials, added in index order from 0.0 with eight loads in flight (one dependent load per
// partial took 72 us for 256 partials)
__device__ __forceinline__ double kf_partial_sum(const double* __restrict__ part, int nb, int tid) {
  double s = 0.0;
  int b = 0;
  for (; b + 8 <= nb; b += 8) {
    double x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = part[(size_t)(b + u) * kfp::kSums + tid];
#pragma unroll
    for (int u = 0; u < 8; ++u) s = s + x[u];
  }
  for (; b < nb; ++b) s = s + part[(size_t)b * kfp::kSums + tid];
  return s;
}
// N per-wave counts of a workgroup of 256 (n: the same in every lane of a wave) added to cnt[0 .. N): lane 0 of each wave leaves them
// in LDS and N threads add the workgroup's non-zero sums with integer atomics (same-address atomics run one after the other at the
// memory side: one set per workgroup, not per wave). sh: 4 x N ints of LDS.
template <int N>
__device__ __forceinline__ void kf_add_counts(const int (&n)[N], int (*sh)[N], int* __restrict__ cnt) {
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) sh[tid >> 6][k] = n[k];
  }
  __syncthreads();
  if (tid < N) {
    const int sum = (sh[0][tid] + sh[1][tid]) + (sh[2][tid] + sh[3][tid]);
    if (sum) atomicAdd(cnt + tid, sum);
  }
}

// One evaluation of the pose's normal equations (kf_pose.hpp: kfp::term is the definition's per-record statement). One thread per
// candidate record of k_kf_emit, the record count and the current pose read from device memory. kf_block_sums leaves one partial of
// 28 doubles and the count of used terms per workgroup. A workgroup behind the last record writes zeros.
__global__ __launch_bounds__(256) void k_kf_pose_sums(KParams p, MapDev m, const float4* __restrict__ rec, const int* __restrict__ count,
                                                      const float4* __restrict__ prs, const unsigned* __restrict__ kf_matches,
                                                      rebvio_hip_cloud_filter flt, double huber, const rebvio_hip_kf_pose* __restrict__ st,
                                                      double* __restrict__ part, int* __restrict__ part_used) {
  __shared__ double sh[4][kfp::kSums];
  __shared__ int sh_used[4];
  const int r = blockIdx.x * 256 + threadIdx.x;
  double v[kfp::kSums];
#pragma unroll
  for (int k = 0; k < kfp::kSums; ++k) v[k] = 0.0;
  bool used = false;
  if (r < *count) {
    const float4 r0 = rec[2 * (size_t)r];  // kf_keyline, keyline, claimants, matches (k_kf_emit: both below their maps' sizes)
    const int j = __float_as_int(r0.x), i = __float_as_int(r0.y);
    const float4 k4 = prs[j];
    const unsigned kmt = kf_matches[j];
    const float2 q = m.pos_img[i];
    const float2 g = m.grad[i];
    double R[9], t[3];
    kf_load_pose(st, R, t);
    bool in;
    used = kfp::filter_pass(flt, k4.z, k4.w, kmt) && kfp::term(p.fm, k4.x, k4.y, k4.z, q.x, q.y, g.x, g.y, R, t, huber, v, &in);
  }
  kf_block_sums<false>(v, used, false, sh, sh_used, nullptr, part, part_used, nullptr);
}

// The end of one evaluation, one workgroup of 64: lane k < 28 adds the nb (<= kMaxRecBlocks) partials of sum k in index order, lane 28
// the used counts; lane 0 then runs kfp::step - H, g, cost, used into the result block, and unless this is the last evaluation the
// 6x6 Cholesky solve and the SE3 update, workspace in LDS.
__global__ __launch_bounds__(64) void k_kf_pose_step(const double* __restrict__ part, const int* __restrict__ part_used, int nb,
                                                     const int* __restrict__ count, int first, int last, int min_used,
                                                     rebvio_hip_kf_pose* __restrict__ st) {
  __shared__ double S[kfp::kSums];
  __shared__ double ws[48];
  __shared__ int sh_used;
  const int tid = threadIdx.x;
  if (tid < kfp::kSums) {
    S[tid] = kf_partial_sum(part, nb, tid);
  } else if (tid == kfp::kSums) {
    int u = 0;
    for (int b = 0; b < nb; ++b) u += part_used[b];
    sh_used = u;
  }
  __syncthreads();
  if (tid == 0) {
    if (first) st->candidates = *count;
    kfp::step(S, sh_used, first, last, min_used, ws, st);
  }
}

void launch_kf_pose_eval(hipStream_t s, const KParams& p, const MapDev& m, int kf_size, const void* records_dev, const int* count_dev,
                         const void* snap_prs, const unsigned* snap_matches, const rebvio_hip_cloud_filter& flt, double huber, int first,
                         int last, int min_used, rebvio_hip_kf_pose* state_dev, double* part, int* part_used) {
  const int nb = div_up(kf_size, 256);  // (the records number at most kf_size <= kmax: nb <= kMaxRecBlocks)
  RH_LAUNCH(k_kf_pose_sums, dim3(nb), dim3(256), 0, s, p, m, reinterpret_cast<const float4*>(records_dev), count_dev,
            reinterpret_cast<const float4*>(snap_prs), snap_matches, flt, huber, (const rebvio_hip_kf_pose*)state_dev, part, part_used);
  RH_LAUNCH(k_kf_pose_step, dim3(1), dim3(64), 0, s, (const double*)part, (const int*)part_used, nb, count_dev, first, last, min_used,
            state_dev);
}

// ---- alignment of a snapshot through a map's distance field (rebvio_hip_kf_snapshot_add_normals, rebvio_hip_map_keyframe_align) --
// k_kf_snapshot_normals: gradient / gradient_norm of the keylines below both sizes (read on the device), zeros in every other slot
// of the launch grid (= the buffer) and where gradient_norm is not > 0. One 8-byte store per lane.
__global__ __launch_bounds__(256) void k_kf_snapshot_normals(MapDev m, const int* __restrict__ snap_n, float2* __restrict__ out) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const float2 g = m.grad[idx];  // bound-free early loads (the arrays are padded to the launch grid)
  const float gn = m.gnorm[idx];
  const int n = min(m.st->n, *snap_n);
  out[idx] = idx < n && gn > 0.0f ? make_float2(g.x / gn, g.y / gn) : make_float2(0.f, 0.f);
}

void launch_kf_snapshot_normals(hipStream_t s, const KParams& p, const MapDev& m, const int* snap_n, void* normals) {
  RH_LAUNCH(k_kf_snapshot_normals, dim3(div_up(p.kmax, 256)), dim3(256), 0, s, m, snap_n, reinterpret_cast<float2*>(normals));
}

// One evaluation of the alignment's normal equations (kf_pose.hpp: kfp::align_term is the definition's per-keyline statement). One
// thread per keyframe keyline: one 16-byte snapshot load and the 8-byte normal, then two dependent gathers - the field cell, then
// pos and unit of its owner together. assoc[j] is written by every thread below kf_size. The reduction is kf_block_sums: one partial
// and one count per workgroup, no atomic.
__global__ __launch_bounds__(256) void k_kf_align_sums(KParams p, MapDev m, int kf_size, const float4* __restrict__ prs,
                                                       const unsigned* __restrict__ kf_matches, const float2* __restrict__ normals,
                                                       rebvio_hip_cloud_filter flt, double huber, double min_cos, int max_dist,
                                                       const rebvio_hip_kf_pose* __restrict__ st, double* __restrict__ part,
                                                       int* __restrict__ part_used, int* __restrict__ assoc) {
  __shared__ double sh[4][kfp::kSums];
  __shared__ int sh_used[4];
  const int j = blockIdx.x * 256 + threadIdx.x;
  double v[kfp::kSums];
#pragma unroll
  for (int k = 0; k < kfp::kSums; ++k) v[k] = 0.0;
  bool used = false;
  if (j < kf_size) {
    const float4 k4 = prs[j];
    const unsigned kmt = kf_matches[j];
    const float2 kn = normals ? normals[j] : make_float2(0.f, 0.f);
    double R[9], t[3];
    kf_load_pose(st, R, t);
    const kfp::AlignMap c = kf_align_map(p, m);
    int i = -1;
    bool in;
    if (kfp::filter_pass(flt, k4.z, k4.w, kmt))
      i = kfp::align_term(c, k4.x, k4.y, k4.z, normals != nullptr, kn.x, kn.y, min_cos, max_dist, R, t, huber, v, &in);
    used = i >= 0;
    assoc[j] = i;
  }
  kf_block_sums<false>(v, used, false, sh, sh_used, nullptr, part, part_used, nullptr);
}

void launch_kf_align_eval(hipStream_t s, const KParams& p, const MapDev& m, int kf_size, const int* kf_size_dev, const void* snap_prs,
                          const unsigned* snap_matches, const void* snap_normals, const rebvio_hip_cloud_filter& flt, double huber,
                          double min_cos, int max_dist, int first, int last, int min_used, rebvio_hip_kf_pose* state_dev, double* part,
                          int* part_used, int* assoc) {
  const int nb = div_up(kf_size, 256);  // (kf_size <= kmax: nb <= kMaxRecBlocks)
  RH_LAUNCH(k_kf_align_sums, dim3(nb), dim3(256), 0, s, p, m, kf_size, reinterpret_cast<const float4*>(snap_prs), snap_matches,
            reinterpret_cast<const float2*>(snap_normals), flt, huber, min_cos, max_dist, (const rebvio_hip_kf_pose*)state_dev, part,
            part_used, assoc);
  RH_LAUNCH(k_kf_pose_step, dim3(1), dim3(64), 0, s, (const double*)part, (const int*)part_used, nb, kf_size_dev, first, last, min_used,
            state_dev);
}

// ---- many hypotheses against one map (rebvio_hip_map_keyframe_align_many) -----------------------------------------------------------
// k_kf_align_sums for a list of (snapshot, pose) hypotheses in one launch: blockIdx.y is the hypothesis, blockIdx.x its workgroup.
// The descriptor (64 bytes at a workgroup-uniform address: scalar loads) names the snapshot's buffers and size and the hypothesis's
// result block and partials. A workgroup behind its own hypothesis's last keyline leaves before any vector load and before the
// barrier - the whole workgroup takes that branch. The per-thread statement is kfp::align_term, here with the Huber test's outcome
// kept, and the reduction is kf_block_sums, k_kf_align_sums' own: a hypothesis's partials are the bits the single kernel writes for
// the same snapshot and pose. The inlier count goes the way of `used`: ballot, popcount, LDS. No assoc is written.
__global__ __launch_bounds__(256) void k_kf_align_sums_many(KParams p, MapDev m, const KfHypDesc* __restrict__ desc,
                                                            rebvio_hip_cloud_filter flt, double huber, double min_cos, int max_dist) {
  __shared__ double sh[4][kfp::kSums];
  __shared__ int sh_used[4];
  __shared__ int sh_inl[4];
  const KfHypDesc d = desc[blockIdx.y];
  if ((int)blockIdx.x * 256 >= d.size) return;
  const float4* __restrict__ prs = reinterpret_cast<const float4*>(d.prs);
  const float2* __restrict__ normals = reinterpret_cast<const float2*>(d.normals);
  const rebvio_hip_kf_pose* __restrict__ st = &d.res->pose;
  const int j = blockIdx.x * 256 + threadIdx.x;
  double v[kfp::kSums];
#pragma unroll
  for (int k = 0; k < kfp::kSums; ++k) v[k] = 0.0;
  bool used = false, inl = false;
  if (j < d.size) {
    const float4 k4 = prs[j];
    const unsigned kmt = d.matches[j];
    const float2 kn = normals ? normals[j] : make_float2(0.f, 0.f);
    double R[9], t[3];
    kf_load_pose(st, R, t);
    const kfp::AlignMap c = kf_align_map(p, m);
    int i = -1;
    bool in = false;
    if (kfp::filter_pass(flt, k4.z, k4.w, kmt))
      i = kfp::align_term(c, k4.x, k4.y, k4.z, normals != nullptr, kn.x, kn.y, min_cos, max_dist, R, t, huber, v, &in);
    used = i >= 0;
    inl = used && in;
  }
  kf_block_sums<true>(v, used, inl, sh, sh_used, sh_inl, d.part, d.part_used, d.part_inl);
}

// k_kf_pose_step for the list, one workgroup of 64 per hypothesis: lane k < 28 adds that hypothesis's first ceil(size / 256)
// partials of sum k in index order from 0.0 (kf_partial_sum, as k_kf_pose_step), lane 28 the used counts, lane 29 the inlier
// counts; lane 0 then runs kfp::step on the hypothesis's result block and leaves the inlier count behind it. A hypothesis of size 0
// is left as the host wrote it.
__global__ __launch_bounds__(64) void k_kf_pose_step_many(const KfHypDesc* __restrict__ desc, int first, int last, int min_used) {
  __shared__ double S[kfp::kSums];
  __shared__ double ws[48];
  __shared__ int sh_used, sh_inl;
  const KfHypDesc d = desc[blockIdx.x];
  if (d.size <= 0) return;
  const int nb = (d.size + 255) >> 8;
  const double* __restrict__ part = d.part;
  const int tid = threadIdx.x;
  if (tid < kfp::kSums) {
    S[tid] = kf_partial_sum(part, nb, tid);
  } else if (tid == kfp::kSums) {
    int u = 0;
    for (int b = 0; b < nb; ++b) u += d.part_used[b];
    sh_used = u;
  } else if (tid == kfp::kSums + 1) {
    int u = 0;
    for (int b = 0; b < nb; ++b) u += d.part_inl[b];
    sh_inl = u;
  }
  __syncthreads();
  if (tid == 0) {
    rebvio_hip_kf_pose* st = &d.res->pose;
    if (first) st->candidates = d.size;
    kfp::step(S, sh_used, first, last, min_used, ws, st);
    d.res->inliers = sh_inl;
  }
}

void launch_kf_align_many_eval(hipStream_t s, const KParams& p, const MapDev& m, const KfHypDesc* desc_dev, int n, int nb_max,
                               const rebvio_hip_cloud_filter& flt, double huber, double min_cos, int max_dist, int first, int last,
                               int min_used) {
  RH_LAUNCH(k_kf_align_sums_many, dim3(nb_max, n), dim3(256), 0, s, p, m, desc_dev, flt, huber, min_cos, max_dist);
  RH_LAUNCH(k_kf_pose_step_many, dim3(n), dim3(64), 0, s, desc_dev, first, last, min_used);
}

// ---- depth fusion into a snapshot (rebvio_hip_kf_snapshot_fuse_depth) ------------------------------------------------------------
// kfp::fuse_term (kf_pose.hpp) is the definition's per-keyline statement. One thread per keyframe keyline, a stride loop behind the
// grid's cap: the 16-byte record, the matches word and the 8-byte normal, then the two dependent gathers of the lookup; a fused
// keyline stores its record and matches word back, every keyline its assoc word. The pose comes as kernel arguments (SGPRs). The
// five counts (associated, fused, gated, flat, clamped) are ballots summed per wave over the loop, which kf_add_counts adds to
// cnt[1..5] - no floating-point value crosses threads. The size is read on the device (behind the snapshot kernel in stream order),
// the stride from the grid.
struct KfFusePose {
  double R[9], t[3];
};
__global__ __launch_bounds__(256) void k_kf_fuse_depth(KParams p, MapDev m, const int* __restrict__ snap_n, float4* __restrict__ prs,
                                                       unsigned* __restrict__ kf_matches, const float2* __restrict__ normals,
                                                       rebvio_hip_cloud_filter flt, double min_cos, int max_dist, KfFusePose pose,
                                                       double pixel_sigma, double gate_sigma, double q_abs, int* __restrict__ cnt,
                                                       int* __restrict__ assoc) {
  __shared__ int sh_cnt[4][5];
  const int tid = threadIdx.x;
  const int n = min(*snap_n, p.kmax), stride = (int)gridDim.x * 256;
  const kfp::AlignMap c = kf_align_map(p, m);
  int nc[5] = {0, 0, 0, 0, 0};
  for (int base = blockIdx.x * 256; base < n; base += stride) {  // (uniform over the workgroup: the ballots see whole waves)
    const int j = base + tid;
    int outcome = kfp::kFuseNone;
    bool clamped = false;
    if (j < n) {
      const float4 k4 = prs[j];
      const unsigned kmt = kf_matches[j];
      const float2 kn = normals ? normals[j] : make_float2(0.f, 0.f);
      int i = 0;
      float rho_n = 0.f, sig_n = 0.f;
      if (kfp::filter_pass(flt, k4.z, k4.w, kmt))
        outcome = kfp::fuse_term(c, k4.x, k4.y, k4.z, k4.w, normals != nullptr, kn.x, kn.y, min_cos, max_dist, pose.R, pose.t, pixel_sigma,
                                 gate_sigma, q_abs, &i, &rho_n, &sig_n, &clamped);
      if (outcome == kfp::kFuseFused) {
        prs[j] = make_float4(k4.x, k4.y, rho_n, sig_n);
        kf_matches[j] = kmt == 0xFFFFFFFFu ? kmt : kmt + 1u;
      } else {
        clamped = false;
      }
      assoc[j] = outcome == kfp::kFuseNone ? (int)0x80000000 : outcome == kfp::kFuseFused ? i : -1 - i;
    }
    nc[0] += __popcll(__ballot(outcome != kfp::kFuseNone));
    nc[1] += __popcll(__ballot(outcome == kfp::kFuseFused));
    nc[2] += __popcll(__ballot(outcome == kfp::kFuseGated));
    nc[3] += __popcll(__ballot(outcome == kfp::kFuseFlat));
    nc[4] += __popcll(__ballot(clamped));
  }
  kf_add_counts(nc, sh_cnt, cnt + 1);
  if (blockIdx.x == 0 && tid == 0) cnt[0] = n;
}

void launch_kf_fuse_depth(hipStream_t s, const KParams& p, const MapDev& m, int kf_size, const int* kf_size_dev, void* snap_prs,
                          unsigned* snap_matches, const void* snap_normals, const rebvio_hip_kf_fuse_opts& o, const double* R, const double* t,
                          int* cnt, int* assoc) {
  KfFusePose pose;
  for (int k = 0; k < 9; ++k) pose.R[k] = R[k];
  for (int k = 0; k < 3; ++k) pose.t[k] = t[k];
  const int want = div_up(kf_size, 256), nb = want < kMaxRecBlocks ? want : kMaxRecBlocks;  // (k_kf_align_sums' cap)
  RH_LAUNCH(k_kf_fuse_depth, dim3(nb), dim3(256), 0, s, p, m, kf_size_dev, reinterpret_cast<float4*>(snap_prs), snap_matches,
            reinterpret_cast<const float2*>(snap_normals), o.kf_filter, o.min_cos, o.max_dist, pose, o.pixel_sigma, o.gate_sigma, o.q_abs, cnt,
            assoc);
}

// ---- point cloud of a snapshot (rebvio_hip_kf_snapshot_point_cloud*) -------------------------------------------------------------
// The compaction of k_cloud_count / k_cloud_emit over a snapshot's buffers (bodies copied, not shared: the map's kernels stay as
// they are): one 16-byte prs load and the matches word per lane, bound-free (the buffers cover the launch grid), the size read on
// the device. kf_cloud.hpp's kfc::record is the per-record statement; a record's gradient_norm is +0.0f (a snapshot keeps none).
__global__ __launch_bounds__(256) void k_kf_cloud_count(const float4* __restrict__ prs, const unsigned* __restrict__ matches,
                                                        const int* __restrict__ n_dev, rebvio_hip_cloud_filter flt,
                                                        int* __restrict__ blk_cnt) {
  __shared__ int sh[4];
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const float4 k = prs[idx];
  const unsigned mt = matches[idx];
  const int n = *n_dev;
  const int2 w = wave_place(idx < n && kfp::filter_pass(flt, k.z, k.w, mt));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = w.y;
  __syncthreads();
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(256) void k_kf_cloud_emit(float fm, const float4* __restrict__ prs, const unsigned* __restrict__ matches,
                                                       const int* __restrict__ n_dev, CloudArgs a, const int* __restrict__ blk_cnt,
                                                       int* __restrict__ count_out, float4* __restrict__ out) {
  __shared__ int sh_w[4], sh_lo[4], sh_all[4];
  const int tid = threadIdx.x, idx = blockIdx.x * 256 + tid, wv = tid >> 6;
  const float4 k = prs[idx];
  const unsigned mt = matches[idx];
  const int n = *n_dev;
  // every workgroup's count, one per thread (gridDim.x <= kMaxRecBlocks = 256)
  const int c = tid < (int)gridDim.x ? blk_cnt[tid] : 0;
  const int lo = wave_sum_i(tid < (int)blockIdx.x ? c : 0), all = wave_sum_i(c);
  const rebvio_hip_cloud_filter flt{a.min_matches, a.max_rel_sigma, a.rho_min, a.rho_max};
  float q[3] = {0.0f, 0.0f, 0.0f};
  const bool pass = kfc::record(fm, flt, a.R, a.t, a.scale, k.x, k.y, k.z, k.w, mt, q) && idx < n;
  const int2 w = wave_place(pass);
  if ((tid & 63) == 0) {
    sh_w[wv] = w.y;
    sh_lo[wv] = lo;
    sh_all[wv] = all;
  }
  __syncthreads();
  int rank = (sh_lo[0] + sh_lo[1]) + (sh_lo[2] + sh_lo[3]) + w.x;
  for (int i = 0; i < wv; ++i) rank += sh_w[i];
  if (blockIdx.x == 0 && tid == 0) *count_out = (sh_all[0] + sh_all[1]) + (sh_all[2] + sh_all[3]);
  if (pass && rank < a.cap) {
    // two 16-byte stores per record, as k_cloud_emit
    typedef float v4f __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(1))) volatile v4f* GRec;
    GRec rec = (GRec)(out + 2 * (size_t)rank);
    rec[0] = v4f{q[0], q[1], q[2], k.z};
    rec[1] = v4f{k.w, 0.0f, __int_as_float(idx), __uint_as_float(mt)};
  }
}

void launch_kf_point_cloud(hipStream_t s, const KParams& p, const void* snap_prs, const unsigned* snap_matches, const int* snap_n,
                           const CloudArgs& a, int* blk_cnt, int* count_dev, void* records_dev) {
  const dim3 grid(div_up(p.kmax, 256));
  const rebvio_hip_cloud_filter flt{a.min_matches, a.max_rel_sigma, a.rho_min, a.rho_max};
  RH_LAUNCH(k_kf_cloud_count, grid, dim3(256), 0, s, reinterpret_cast<const float4*>(snap_prs), snap_matches, snap_n, flt, blk_cnt);
  RH_LAUNCH(k_kf_cloud_emit, grid, dim3(256), 0, s, p.fm, reinterpret_cast<const float4*>(snap_prs), snap_matches, snap_n, a,
            (const int*)blk_cnt, count_dev, reinterpret_cast<float4*>(records_dev));
}

// ---- depth hand-over between snapshots (rebvio_hip_kf_snapshot_handover_depth) -----------------------------------------------------
// kfp::handover_claim_term / handover_apply_term (kf_handover.hpp) are the definition's per-keyline statements.
//   k_kf_handover_claim  one thread per src keyline, a stride loop behind the grid's cap, as k_kf_fuse_depth: the 16-byte record,
//                        the matches word and the 8-byte normal, then the dependent gathers of the lookup (the field's cell, the
//                        owner's unit). A surviving keyline stores its 8-byte staging record (rho_c, matches; the bits of sig_c ride
//                        in the key) and issues ONE 64-bit atomicMin on its owner's claim word: independent of the order the claims
//                        arrive in. Claimants of one owner hit one address and are served one after the other at the memory side -
//                        the price of a collision, paid only by the colliding keylines; the atomic returns nothing the thread waits
//                        for. Every keyline writes its assoc word: INT_MIN when not associated, -1 - i otherwise - the word of every
//                        outcome but one, the winner of an adopted slot, which the apply pass overwrites (stream order puts that
//                        store behind this one). So no pass compares a loser's key with its slot's.
//   k_kf_handover_apply  one thread per dst keyline, the same cap and loop: the claim word, nothing more for an empty slot; else the
//                        winner's staging record (one 8-byte gather) and the slot's record and matches word; steps 4..6.
// Counts: ballots summed per wave over the loop, then kf_add_counts (associated, out of range -> cnt[1..2]; claimed, adopted, kept,
// conflict -> cnt[3..6]). No floating-point value crosses threads. Sizes are read on the device.
__global__ __launch_bounds__(256) void k_kf_handover_claim(KParams p, MapDev m, const int* __restrict__ src_n, const int* __restrict__ dst_n,
                                                           const float4* __restrict__ prs, const unsigned* __restrict__ kf_matches,
                                                           const float2* __restrict__ normals, rebvio_hip_cloud_filter flt, double min_cos,
                                                           int max_dist, KfFusePose pose, double q_abs,
                                                           unsigned long long* __restrict__ key, kfp::HandoverStage* __restrict__ stage,
                                                           int* __restrict__ cnt, int* __restrict__ assoc) {
  __shared__ int sh_cnt[4][2];
  const int tid = threadIdx.x;
  const int n = min(*src_n, p.kmax), nd = min(*dst_n, p.kmax), stride = (int)gridDim.x * 256;
  const kfp::AlignMap c = kf_align_map(p, m);
  int nc[2] = {0, 0};
  for (int base = blockIdx.x * 256; base < n; base += stride) {  // (uniform over the workgroup: the ballots see whole waves)
    const int j = base + tid;
    int outcome = kfp::kHoNone;
    if (j < n) {
      const float4 k4 = prs[j];
      const unsigned kmt = kf_matches[j];
      const float2 kn = normals ? normals[j] : make_float2(0.f, 0.f);
      int i = 0;
      float rho_c = 0.f, sig_c = 0.f;
      if (kfp::filter_pass(flt, k4.z, k4.w, kmt))
        outcome = kfp::handover_claim_term(c, nd, k4.x, k4.y, k4.z, k4.w, normals != nullptr, kn.x, kn.y, min_cos, max_dist, pose.R, pose.t,
                                           q_abs, &i, &rho_c, &sig_c);
      if (outcome == kfp::kHoClaim) {  // (i < nd <= kmax, j < n <= kmax: inside the scratch)
        stage[j] = kfp::HandoverStage{rho_c, kmt};
        atomicMin(key + i, kfp::handover_key(sig_c, j));
      }
      assoc[j] = outcome == kfp::kHoNone ? (int)0x80000000 : -1 - i;
    }
    nc[0] += __popcll(__ballot(outcome != kfp::kHoNone));
    nc[1] += __popcll(__ballot(outcome == kfp::kHoOutOfRange));
  }
  kf_add_counts(nc, sh_cnt, cnt + 1);
  if (blockIdx.x == 0 && tid == 0) cnt[0] = n;
}

__global__ __launch_bounds__(256) void k_kf_handover_apply(int kmax, const int* __restrict__ src_n, const int* __restrict__ dst_n,
                                                           float4* __restrict__ prs, unsigned* __restrict__ dst_matches, double gate_sigma,
                                                           const unsigned long long* __restrict__ key,
                                                           const kfp::HandoverStage* __restrict__ stage, int* __restrict__ cnt,
                                                           int* __restrict__ assoc) {
  __shared__ int sh_cnt[4][4];
  const int tid = threadIdx.x;
  const int n = min(*src_n, kmax), nd = min(*dst_n, kmax), stride = (int)gridDim.x * 256;
  int nc[4] = {0, 0, 0, 0};
  for (int base = blockIdx.x * 256; base < nd; base += stride) {
    const int i = base + tid;
    int slot = kfp::kHoEmpty;
    if (i < nd) {
      const unsigned long long k = key[i];
      const int win = (int)(unsigned)k;
      if (k != kfp::kHoEmptyKey && win < n) {  // (a claimant's index is below src's size: the test only keeps the gather inside)
        const kfp::HandoverStage st = stage[win];
        const float4 d4 = prs[i];
        const unsigned dmt = dst_matches[i];
        unsigned mt_n = dmt;
        const float sc = kfp::handover_key_sigma(k);
        slot = kfp::handover_apply_term(st.rho_c, sc, st.matches, d4.z, d4.w, dmt, gate_sigma, &mt_n);
        if (slot == kfp::kHoAdopted) {
          prs[i] = make_float4(d4.x, d4.y, st.rho_c, sc);
          dst_matches[i] = mt_n;
          assoc[win] = i;
        }
      }
    }
    nc[0] += __popcll(__ballot(slot != kfp::kHoEmpty));
    nc[1] += __popcll(__ballot(slot == kfp::kHoAdopted));
    nc[2] += __popcll(__ballot(slot == kfp::kHoKept));
    nc[3] += __popcll(__ballot(slot == kfp::kHoConflict));
  }
  kf_add_counts(nc, sh_cnt, cnt + 3);
}

void launch_kf_handover(hipStream_t s, const KParams& p, const MapDev& m, int src_size, const int* src_size_dev, int dst_size,
                        const int* dst_size_dev, const void* src_prs, const unsigned* src_matches, const void* src_normals, void* dst_prs,
                        unsigned* dst_matches, const rebvio_hip_kf_handover_opts& o, const double* R, const double* t,
                        unsigned long long* key, void* stage, int* cnt, int* assoc) {
  KfFusePose pose;
  for (int k = 0; k < 9; ++k) pose.R[k] = R[k];
  for (int k = 0; k < 3; ++k) pose.t[k] = t[k];
  const int want = div_up(src_size, 256), nb = want < kMaxRecBlocks ? want : kMaxRecBlocks;  // (k_kf_fuse_depth's cap)
  RH_LAUNCH(k_kf_handover_claim, dim3(nb), dim3(256), 0, s, p, m, src_size_dev, dst_size_dev, reinterpret_cast<const float4*>(src_prs),
            src_matches, reinterpret_cast<const float2*>(src_normals), o.kf_filter, o.min_cos, o.max_dist, pose, o.q_abs, key,
            reinterpret_cast<kfp::HandoverStage*>(stage), cnt, assoc);
  const int want_d = div_up(dst_size > 0 ? dst_size : 1, 256), nbd = want_d < kMaxRecBlocks ? want_d : kMaxRecBlocks;
  RH_LAUNCH(k_kf_handover_apply, dim3(nbd), dim3(256), 0, s, p.kmax, src_size_dev, dst_size_dev, reinterpret_cast<float4*>(dst_prs),
            dst_matches, o.gate_sigma, (const unsigned long long*)key, reinterpret_cast<const kfp::HandoverStage*>(stage), cnt, assoc);
}

// ---- edge chains and polylines (rebvio_hip_map_edge_chains / rebvio_hip_map_edge_polylines) ----------------------------------------
// List ranking over succ / pred by pointer jumping; ech::* (edge_chains.hpp) are the definition's per-keyline statements. One thread
// per keyline (or slot), ceil(kmax / 256) workgroups per launch, the map's size read on the device. No workgroup waits for another:
// every dependency between workgroups is a kernel boundary.
//   k_chain_link   succ, and the first state of every keyline from pred; workgroup 0 leaves the size and the "moved" words
//   k_chain_round  x ceil(log2(kmax)): state k + 1 of every keyline from state k of itself and of its ancestor (two buffers, all reads
//                  from the previous one). A round stores words[8 + k + 1] = 1 when a state changed (every writer stores the same
//                  value); the round behind one that changed nothing returns at once: that round copied every state as it was, so
//                  both buffers hold the final states whichever round was the last to run.
//   k_chain_rank   head, rank, cyclic per keyline; the chain's last member - one writer per chain - stores rank + 1 as len[head]
//   k_chain_count  length per keyline (len[head]); per workgroup the number of heads and the sum of their lengths
//   k_chain_emit   the two fixed-order integer scans over the head flags: chain number and first slot of every head -> starts, start_of
//   k_chain_order  order[start_of[head] + rank] = keyline: a scatter, one writer per slot
//   k_poly_count / k_poly_emit / k_poly_lines  kept and line-begin flags per slot in one pass, their scans, points and line records;
//                  the last kernel turns a line's (first point, end) into its number of points and its "closed" bit
// No atomics at all; every sum is an integer sum in a fixed order.
__device__ __forceinline__ int chain_size(const MapDev& m, int kmax) {
  const int n = m.st->n;
  return n < 0 ? 0 : (n < kmax ? n : kmax);
}
// (sum of blk[0 .. blockIdx.x), sum of all gridDim.x <= kMaxRecBlocks entries); sh = 8 ints of LDS; ends behind a barrier
__device__ __forceinline__ int2 chain_blk_sums(const int* __restrict__ blk, int* sh) {
  const int tid = threadIdx.x;
  const int c = tid < (int)gridDim.x ? blk[tid] : 0;
  const int lo = wave_sum_i(tid < (int)blockIdx.x ? c : 0), all = wave_sum_i(c);
  if ((tid & 63) == 0) {
    sh[tid >> 6] = lo;
    sh[4 + (tid >> 6)] = all;
  }
  __syncthreads();
  return make_int2((sh[0] + sh[1]) + (sh[2] + sh[3]), (sh[4] + sh[5]) + (sh[6] + sh[7]));
}
// exclusive prefix of v over the workgroup's 256 threads in thread order; sh = 4 ints of LDS; ends behind a barrier
__device__ __forceinline__ int chain_block_scan(int v, int* sh) {
  const int tid = threadIdx.x, lane = tid & 63;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  if (lane == 63) sh[tid >> 6] = x;
  __syncthreads();
  int base = 0;
  for (int k = 0; k < (tid >> 6); ++k) base += sh[k];
  return base + x - v;
}
// the workgroup's sum of v -> out[blockIdx.x]; sh = 4 ints of LDS; ends behind a barrier
__device__ __forceinline__ void chain_block_sum(int v, int* sh, int* __restrict__ out) {
  const int s = wave_sum_i(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(256) void k_chain_link(int kmax, MapDev m, ChainDev c, int rounds) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int n = chain_size(m, kmax);
  if (blockIdx.x == 0 && (int)threadIdx.x <= rounds) {
    if (threadIdx.x == 0) c.words[0] = n;
    c.words[8 + threadIdx.x] = threadIdx.x == 0 ? 1 : 0;
  }
  if (idx >= n) return;
  c.succ[idx] = ech::chain_succ(m.id_prev, m.id_next, n, idx);
  reinterpret_cast<ech::ChainNode*>(c.node[0])[idx] = ech::chain_init(idx, ech::chain_pred(m.id_prev, m.id_next, n, idx));
}

__global__ __launch_bounds__(256) void k_chain_round(ChainDev c, int k) {
  if (c.words[8 + k] == 0) return;  // nothing moved in the round in front: both buffers hold the final states
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int n = c.words[0];
  const ech::ChainNode* in = reinterpret_cast<const ech::ChainNode*>(c.node[k & 1]);
  ech::ChainNode* out = reinterpret_cast<ech::ChainNode*>(c.node[(k + 1) & 1]);
  bool moved = false;
  if (idx < n) out[idx] = ech::chain_round(in, idx, n, &moved);
  if (__ballot(moved) != 0ull && (threadIdx.x & 63) == 0) c.words[8 + k + 1] = 1;
}

__global__ __launch_bounds__(256) void k_chain_rank(ChainDev c, int rounds) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int n = c.words[0];
  if (idx >= n) return;
  int head, rank, cyc;
  ech::chain_resolve(reinterpret_cast<const ech::ChainNode*>(c.node[rounds & 1]), idx, &head, &rank, &cyc);
  c.refs[idx] = rebvio_hip_chain_ref{head, rank, 0, cyc};
  if (ech::chain_is_last(c.succ[idx], head)) c.len[head] = rank + 1;
}

__global__ __launch_bounds__(256) void k_chain_count(ChainDev c) {
  __shared__ int sh[8];
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int n = c.words[0];
  int is_head = 0, len = 0;
  if (idx < n) {
    const int head = c.refs[idx].head;
    len = c.len[head];
    c.refs[idx].length = len;
    is_head = head == idx;
  }
  chain_block_sum(is_head, sh, c.blk);
  chain_block_sum(is_head ? len : 0, sh + 4, c.blk + kMaxRecBlocks);
}

__global__ __launch_bounds__(256) void k_chain_emit(ChainDev c) {
  __shared__ int sh[24];
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int n = c.words[0];
  int is_head = 0, len = 0;
  if (idx < n) {
    const rebvio_hip_chain_ref r = c.refs[idx];
    is_head = r.head == idx;
    len = is_head ? r.length : 0;
  }
  const int2 heads = chain_blk_sums(c.blk, sh);
  const int2 lens = chain_blk_sums(c.blk + kMaxRecBlocks, sh + 8);
  const int cno = heads.x + chain_block_scan(is_head, sh + 16);
  const int start = lens.x + chain_block_scan(len, sh + 20);
  if (is_head) {  // (cno < chains <= n, start < n)
    c.starts[cno] = start;
    c.start_of[idx] = start;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    c.words[1] = heads.y;
    c.starts[heads.y] = n;
  }
}

__global__ __launch_bounds__(256) void k_chain_order(ChainDev c) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int n = c.words[0];
  if (idx >= n) return;
  const rebvio_hip_chain_ref r = c.refs[idx];
  const int slot = c.start_of[r.head] + r.rank;
  if ((unsigned)slot < (unsigned)n) c.order[slot] = idx;  // (always: the test only keeps the scatter inside)
}

// kept / begin / end of slot s < n (k = its keyline, r = its record)
__device__ __forceinline__ bool poly_slot_kept(const MapDev& m, const rebvio_hip_cloud_filter& f, int min_len, int k, int length) {
  const float2 rs = m.rs[k];
  return ech::poly_kept(f, min_len, rs.x, rs.y, m.matches[k], length);
}

__global__ __launch_bounds__(256) void k_poly_count(MapDev m, ChainDev c, rebvio_hip_cloud_filter f, int min_len) {
  __shared__ int sh[8];
  const int s = blockIdx.x * 256 + threadIdx.x;
  const int n = c.words[0];
  int kept = 0, begin = 0;
  if (s < n) {
    const int k = c.order[s];
    const rebvio_hip_chain_ref r = c.refs[k];
    kept = poly_slot_kept(m, f, min_len, k, r.length);
    begin = kept && (r.rank == 0 || !poly_slot_kept(m, f, min_len, c.order[s - 1], r.length));
  }
  chain_block_sum(kept, sh, c.blk + 2 * kMaxRecBlocks);
  chain_block_sum(begin, sh + 4, c.blk + 3 * kMaxRecBlocks);
}

__global__ __launch_bounds__(256) void k_poly_emit(KParams p, MapDev m, ChainDev c, CloudArgs a, int min_len, int cap_lines) {
  __shared__ int sh[24];
  const int s = blockIdx.x * 256 + threadIdx.x;
  const int n = c.words[0];
  const rebvio_hip_cloud_filter f{a.min_matches, a.max_rel_sigma, a.rho_min, a.rho_max};
  int kept = 0, begin = 0, end = 0, k = 0;
  rebvio_hip_chain_ref r{0, 0, 0, 0};
  if (s < n) {
    k = c.order[s];
    r = c.refs[k];
    kept = poly_slot_kept(m, f, min_len, k, r.length);
    begin = kept && (r.rank == 0 || !poly_slot_kept(m, f, min_len, c.order[s - 1], r.length));
    end = kept && !(r.rank + 1 < r.length && poly_slot_kept(m, f, min_len, c.order[s + 1], r.length));
  }
  const int2 pts = chain_blk_sums(c.blk + 2 * kMaxRecBlocks, sh);
  const int2 lns = chain_blk_sums(c.blk + 3 * kMaxRecBlocks, sh + 8);
  const int pidx = pts.x + chain_block_scan(kept, sh + 16);
  const int lidx = lns.x + chain_block_scan(begin, sh + 20) + begin - 1;  // the line of a kept slot: begins up to and with it, less one
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    c.words[2] = pts.y;
    c.words[3] = lns.y;
  }
  if (!kept) return;
  if (pidx < a.cap) {
    const float2 pi = m.pos_img[k];
    const float2 rs = m.rs[k];
    float q[3];
    ech::poly_xyz(p.fm, a.R, a.t, a.scale, pi.x, pi.y, rs.x, q);
    // two 16-byte stores per record, as k_cloud_emit
    typedef float v4f __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(1))) volatile v4f* GRec;
    GRec rec = (GRec)(reinterpret_cast<float4*>(c.points) + 2 * (size_t)pidx);
    rec[0] = v4f{q[0], q[1], q[2], rs.x};
    rec[1] = v4f{rs.y, m.gnorm[k], __int_as_float(k), __uint_as_float(m.matches[k])};
    c.refs2[pidx] = make_int2(r.head, r.rank);
  }
  if (lidx >= 0 && lidx < cap_lines) {  // the line's first and last slot fill its record between them (ech::poly_line_finish ends it)
    if (begin) {
      c.lines[lidx].first_point = pidx;
      c.lines[lidx].head = r.head;
      c.lines[lidx].flags = (r.flags & 1) ? r.length : 0;
    }
    if (end) c.lines[lidx].points = pidx + 1;
  }
}

__global__ __launch_bounds__(256) void k_poly_lines(ChainDev c, int cap_lines) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  const int nl = c.words[3];
  if (l >= nl || l >= cap_lines) return;
  rebvio_hip_polyline rec = c.lines[l];
  ech::poly_line_finish(&rec);
  c.lines[l] = rec;
}

void launch_edge_chains(hipStream_t s, const KParams& p, const MapDev& m, const ChainDev& c, int rounds) {
  const dim3 grid(div_up(p.kmax, 256));
  RH_LAUNCH(k_chain_link, grid, dim3(256), 0, s, p.kmax, m, c, rounds);
  for (int k = 0; k < rounds; ++k) RH_LAUNCH(k_chain_round, grid, dim3(256), 0, s, c, k);
  RH_LAUNCH(k_chain_rank, grid, dim3(256), 0, s, c, rounds);
  RH_LAUNCH(k_chain_count, grid, dim3(256), 0, s, c);
  RH_LAUNCH(k_chain_emit, grid, dim3(256), 0, s, c);
  RH_LAUNCH(k_chain_order, grid, dim3(256), 0, s, c);
}

void launch_edge_polylines(hipStream_t s, const KParams& p, const MapDev& m, const ChainDev& c, const CloudArgs& a, int min_chain_length,
                           int cap_lines) {
  const dim3 grid(div_up(p.kmax, 256));
  const rebvio_hip_cloud_filter f{a.min_matches, a.max_rel_sigma, a.rho_min, a.rho_max};
  RH_LAUNCH(k_poly_count, grid, dim3(256), 0, s, m, c, f, min_chain_length);
  RH_LAUNCH(k_poly_emit, grid, dim3(256), 0, s, p, m, c, a, min_chain_length, cap_lines);
  RH_LAUNCH(k_poly_lines, grid, dim3(256), 0, s, c, cap_lines);
}

// ---- straight segments of the polylines (rebvio_hip_map_edge_segments) ---------------------------------------------------------------
// Breadth-first Douglas-Peucker over the polylines' points and a weighted line fit of inverse depth per kept segment; esg::*
// (edge_segments.hpp) are the definition's per-point statements. One thread per point, ceil(kmax / 256) workgroups per launch (the
// fit: 16 lanes per segment), the counts read on the device. No workgroup waits for another: every dependency is a kernel boundary.
//   k_seg_init   the point (pos_img, rho, sigma_rho) next to its state: its line by bisection over the line records, the first
//                span, nxt of a vertex = the end of the segment it begins; both far buffers' own slot cleared; workgroup 0 leaves the
//                counts and the "split" words
//   k_seg_far    x (max_rounds + 1): every interior point forms its key; a wave's lanes are in point order, so lanes of one segment
//                are a run of equal `a`: a segmented maximum over the run (shuffles), then ONE 64-bit atomicMax per (wave, segment) on
//                far[k & 1][a]. The keys are distinct: the maximum does not depend on the order it is taken in.
//   k_seg_split  x max_rounds: the point reads its segment's winner and takes its new span; the winner stores nxt[a] = m,
//                nxt[m] = b and words[8 + k + 1] = 1; every point clears its own slot of the OTHER far buffer for the round behind.
//                A far / split behind a round in which nothing split returns at once: far[rounds_used & 1] holds every segment's
//                final measure whichever pass was the last to run.
//   k_seg_count / k_seg_emit  segment, kept and unresolved flags per segment start, their fixed-order scans, the list of kept starts
//   k_seg_fit    one 16-lane row per kept segment (four per wave): lane j forms partial j of the six sums, the xor-1, 2, 4, 8
//                butterfly inside the row is the definition's pairwise tree (a + b == b + a bit for bit), lane 0 stores the record
// The only floating-point values that cross threads are the keys (a maximum) and the partials (a fixed tree).
__device__ __forceinline__ int seg_rounds_used(const int* __restrict__ words, int max_rounds) {
  int ru = 0;
  for (int k = 1; k <= max_rounds; ++k) ru += words[8 + k];
  return ru;
}

__global__ __launch_bounds__(256) void k_seg_init(MapDev m, ChainDev c, SegDev g) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int np = c.words[2], nl = c.words[3];
  if (blockIdx.x == 0 && (int)threadIdx.x < esg::kSegWords)
    g.words[threadIdx.x] = threadIdx.x == 0 ? np : (threadIdx.x == 1 ? nl : (threadIdx.x == 8 ? 1 : 0));
  if (p >= np || nl <= 0) return;
  int lo = 0, hi = nl - 1;  // the last line that begins at or in front of p
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (c.lines[mid].first_point <= p) lo = mid; else hi = mid - 1;
  }
  const rebvio_hip_polyline ln = c.lines[lo];
  const int first = ln.first_point, last = first + ln.points - 1;
  const float4* rec = reinterpret_cast<const float4*>(c.points) + 2 * (size_t)p;
  const float4 r0 = rec[0], r1 = rec[1];
  const float2 pi = m.pos_img[__float_as_int(r1.z)];
  reinterpret_cast<esg::SegPoint*>(g.q)[p] = esg::SegPoint{pi.x, pi.y, r0.w, r1.x};
  const bool vertex = p <= first || p >= last;
  reinterpret_cast<esg::SegSpan*>(g.span)[p] = vertex ? esg::SegSpan{p, p} : esg::SegSpan{first, last};
  g.nxt[p] = (p == first && last > first) ? last : p;
  g.line_of[p] = lo;
  g.far[0][p] = 0ull;
  g.far[1][p] = 0ull;
}

__global__ __launch_bounds__(256) void k_seg_far(SegDev g, int k) {
  if (g.words[8 + k] == 0) return;  // nothing split in the round in front: the measures stand
  const int p = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  const int np = g.words[0];
  const esg::SegPoint* q = reinterpret_cast<const esg::SegPoint*>(g.q);
  int id = 0x7FFFFFFF;  // a vertex joins the run of the segment it begins with key 0
  unsigned long long key = 0ull;
  if (p < np) {
    const esg::SegSpan s = reinterpret_cast<const esg::SegSpan*>(g.span)[p];
    id = s.a;
    if (s.a != p) key = esg::seg_key(esg::seg_dev2(q[s.a], q[s.b], q[p]), p);
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {  // the maximum of the run up to and with this lane (ids ascend along the wave)
    const int id_o = __shfl_up(id, o);
    const unsigned long long key_o = __shfl_up(key, o);
    if (lane >= o && id_o == id && key_o > key) key = key_o;
  }
  const int id_n = __shfl_down(id, 1);
  if ((lane == 63 || id_n != id) && key != 0ull) atomicMax(&g.far[k & 1][id], key);
}

__global__ __launch_bounds__(256) void k_seg_split(SegDev g, int k, float tol2) {
  if (g.words[8 + k] == 0) return;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int np = g.words[0];
  bool won = false;
  if (p < np) {
    g.far[(k + 1) & 1][p] = 0ull;
    esg::SegSpan* span = reinterpret_cast<esg::SegSpan*>(g.span);
    const esg::SegSpan s = span[p];
    if (s.a != p) {
      const esg::SegSpan t = esg::seg_split(s, p, g.far[k & 1][s.a], tol2, &won);
      if (t.a != s.a || t.b != s.b) span[p] = t;
      if (won) {
        g.nxt[s.a] = p;
        g.nxt[p] = s.b;
      }
    }
  }
  if (__ballot(won) != 0ull && (threadIdx.x & 63) == 0) g.words[8 + k + 1] = 1;
}

// segment / kept / unresolved of point p < np
__device__ __forceinline__ void seg_flags(const SegDev& g, const SegArgs& sa, const unsigned long long* __restrict__ far, int p, int* is_seg,
                                          int* kept, int* unres) {
  const esg::SegPoint* q = reinterpret_cast<const esg::SegPoint*>(g.q);
  const int b = g.nxt[p];
  *is_seg = reinterpret_cast<const esg::SegSpan*>(g.span)[p].a == p && b != p;
  *kept = *unres = 0;
  if (!*is_seg) return;
  *unres = esg::key_splits(far[p], sa.tol2);
  *kept = esg::seg_kept(b - p + 1, esg::seg_l2(q[p], q[b]), sa.min_points, sa.min_len2);
}

__global__ __launch_bounds__(256) void k_seg_count(SegDev g, SegArgs sa) {
  __shared__ int sh[12];
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int np = g.words[0];
  int is_seg = 0, kept = 0, unres = 0;
  if (p < np) seg_flags(g, sa, g.far[seg_rounds_used(g.words, sa.max_rounds) & 1], p, &is_seg, &kept, &unres);
  chain_block_sum(is_seg, sh, g.blk);
  chain_block_sum(kept, sh + 4, g.blk + kMaxRecBlocks);
  chain_block_sum(unres, sh + 8, g.blk + 2 * kMaxRecBlocks);
}

__global__ __launch_bounds__(256) void k_seg_emit(SegDev g, SegArgs sa) {
  __shared__ int sh[28];
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int np = g.words[0];
  const int ru = seg_rounds_used(g.words, sa.max_rounds);
  int is_seg = 0, kept = 0, unres = 0;
  if (p < np) seg_flags(g, sa, g.far[ru & 1], p, &is_seg, &kept, &unres);
  const int2 alls = chain_blk_sums(g.blk, sh);
  const int2 kepts = chain_blk_sums(g.blk + kMaxRecBlocks, sh + 8);
  const int2 unress = chain_blk_sums(g.blk + 2 * kMaxRecBlocks, sh + 16);
  const int idx = kepts.x + chain_block_scan(kept, sh + 24);
  if (kept) g.seg[idx] = p;  // (idx < kept segments < np)
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    g.words[2] = alls.y;
    g.words[3] = kepts.y;
    g.words[4] = 0;  // depth valid: k_seg_fit counts
    g.words[5] = unress.y;
    g.words[6] = ru;
  }
}

__global__ __launch_bounds__(256) void k_seg_fit(KParams p, SegDev g, CloudArgs a, SegArgs sa) {
  const int row = threadIdx.x >> 4, j = threadIdx.x & (esg::kLanes - 1);
  const int n_kept = g.words[3];
  const esg::SegPoint* q = reinterpret_cast<const esg::SegPoint*>(g.q);
  const unsigned long long* far = g.far[g.words[6] & 1];
  for (int i = blockIdx.x * 16 + row; i < n_kept; i += gridDim.x * 16) {
    const int a0 = g.seg[i], b = g.nxt[a0], points = b - a0 + 1;
    const esg::SegPoint qa = q[a0], qb = q[b];
    const float l2 = esg::seg_l2(qa, qb);
    esg::FitSums f = esg::fit_zero();
    for (int mbr = j; mbr < points; mbr += esg::kLanes) esg::fit_add(&f, qa, qb, l2, q[a0 + mbr]);
#pragma unroll
    for (int w = 1; w < esg::kLanes; w <<= 1) {
      esg::FitSums o;
#pragma unroll
      for (int k = 0; k < 6; ++k) o.s[k] = __shfl_xor(f.s[k], w);
      f = esg::fit_pair(f, o);
    }
    if (j != 0) continue;
    const unsigned long long key = far[a0];
    const rebvio_hip_line_segment rec = esg::fit_finish(f, qa, qb, esg::key_dev2(key), a0, points, g.line_of[a0], esg::key_splits(key, sa.tol2),
                                                        p.fm, a.R, a.t, a.scale, a.rho_min, a.rho_max);
    // five 16-byte stores per record
    typedef float v4f __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(1))) volatile v4f* GRec;
    GRec out = (GRec)(reinterpret_cast<float4*>(g.recs) + 5 * (size_t)i);
    out[0] = v4f{rec.xyz0[0], rec.xyz0[1], rec.xyz0[2], rec.xyz1[0]};
    out[1] = v4f{rec.xyz1[1], rec.xyz1[2], rec.uv0[0], rec.uv0[1]};
    out[2] = v4f{rec.uv1[0], rec.uv1[1], rec.rho0, rec.rho1};
    out[3] = v4f{rec.sigma_rho0, rec.sigma_rho1, rec.max_dev2, rec.chi2};
    out[4] = v4f{__int_as_float(rec.first_point), __int_as_float(rec.points), __int_as_float(rec.line), __int_as_float(rec.flags)};
    if (rec.flags & 1) atomicAdd(&g.words[4], 1);
  }
}

void launch_edge_segments(hipStream_t s, const KParams& p, const MapDev& m, const ChainDev& c, const SegDev& g, const CloudArgs& a,
                          const SegArgs& sa) {
  const dim3 grid(div_up(p.kmax, 256));
  RH_LAUNCH(k_seg_init, grid, dim3(256), 0, s, m, c, g);
  for (int k = 0; k < sa.max_rounds; ++k) {
    RH_LAUNCH(k_seg_far, grid, dim3(256), 0, s, g, k);
    RH_LAUNCH(k_seg_split, grid, dim3(256), 0, s, g, k, sa.tol2);
  }
  RH_LAUNCH(k_seg_far, grid, dim3(256), 0, s, g, sa.max_rounds);
  RH_LAUNCH(k_seg_count, grid, dim3(256), 0, s, g, sa);
  RH_LAUNCH(k_seg_emit, grid, dim3(256), 0, s, g, sa);
  // the fit: 16 rows per workgroup, i.e. one row per 16 points at once (kept segments of min_points >= 2 number fewer than the
  // points; the default min_points 8 leaves at most one per 7); the stride loop covers what is left
  RH_LAUNCH(k_seg_fit, grid, dim3(256), 0, s, p, g, a, sa);
}

// ---- depth prior from a registered depth image (rebvio_hip_map_fuse_depth_image*) --------------------------------------------------
// dpr::term (depth_prior.hpp) is the definition's per-keyline statement. One thread per keyline, the map's size read on the device:
// pos, gradient, gradient_norm and (rho, sigma_rho) from the SoA arrays, up to three gathered taps of 2 or 4 bytes, the pair stored
// back where the keyline is fused, the outcome word for every keyline. The image and the options come as kernel arguments (SGPRs).
// The five counts (sampled, fused, gated, jumps, clamped) are ballots per wave, which kf_add_counts adds to cnt[1..5] - integer
// sums, no floating-point value crosses threads. Slots behind the size get outcome 0.
__global__ __launch_bounds__(256) void k_depth_prior(KParams p, MapDev m, dpr::Args a, int* __restrict__ cnt, int* __restrict__ outcome) {
  __shared__ int sh_cnt[4][5];
  const int tid = threadIdx.x;
  const int n = min(max(m.st->n, 0), p.kmax);
  const int i = blockIdx.x * 256 + tid;
  int oc = dpr::kNone;
  if (i < n) {
    const float2 pos = m.pos[i], g = m.grad[i], rs = m.rs[i];
    const float gn = m.gnorm[i];
    float rho_n = 0.f, sig_n = 0.f;
    oc = dpr::term(a, pos.x, pos.y, g.x, g.y, gn, rs.x, rs.y, &rho_n, &sig_n);
    if ((oc & 3) == dpr::kFused) m.rs[i] = make_float2(rho_n, sig_n);
  }
  if (i < p.kmax) outcome[i] = oc;
  int nc[5];
  nc[0] = __popcll(__ballot(oc != dpr::kNone));
  nc[1] = __popcll(__ballot((oc & 3) == dpr::kFused));
  nc[2] = __popcll(__ballot((oc & 3) == dpr::kGated));
  nc[3] = __popcll(__ballot((oc & dpr::kJumpBit) != 0));
  nc[4] = __popcll(__ballot((oc & dpr::kClampedBit) != 0));
  kf_add_counts(nc, sh_cnt, cnt + 1);
  if (blockIdx.x == 0 && tid == 0) cnt[0] = n;
}

void launch_depth_prior(hipStream_t s, const KParams& p, const MapDev& m, const dpr::Args& a, int* cnt, int* outcome) {
  RH_LAUNCH(k_depth_prior, dim3(div_up(p.kmax, 256)), dim3(256), 0, s, p, m, a, cnt, outcome);
}

// ---- depth prior from a rectified stereo partner's edge map (rebvio_hip_map_fuse_stereo*) ---------------------------------------------
// stereo_prior.hpp holds the definition's statements. A sub-group of kSprLanes lanes serves one left keyline (256 / kSprLanes
// keylines per workgroup, the sizes of both maps read on the device): every lane loads the keyline and runs spr::left_setup, the
// lanes then take consecutive columns of the window's rows in the right map's mask - one coalesced read per row and step - and a
// lane that meets a keyline gathers its pos, gradient and gradient_norm and folds it (spr::fold_candidate). The folds meet in a
// butterfly of __shfl_xor inside the sub-group: an OR, a minimum, a maximum and the smallest (score, j), none of which depends on
// the order - every lane ends with the same fold, and lane 0 decides, updates and stores. A mask word outside [0, right size) is
// no keyline. The six counts (usable, seen, fused, gated, ambiguous, clamped) are ballots per wave over the sub-groups' lanes 0,
// which kf_add_counts adds to cnt[1..6]. Slots behind the size get outcome 0, winner -1.
#ifndef RH_SPR_LANES
#define RH_SPR_LANES 16
#endif
constexpr int kSprLanes = RH_SPR_LANES;
static_assert(kSprLanes == 4 || kSprLanes == 8 || kSprLanes == 16 || kSprLanes == 32 || kSprLanes == 64, "a power of two inside a wave");
__global__ __launch_bounds__(256) void k_stereo_prior(KParams p, MapDev m, MapDev r, int r_kmax, spr::Args a, int* __restrict__ cnt,
                                                      int* __restrict__ outcome, int* __restrict__ winner) {
  __shared__ int sh_cnt[4][6];
  const int tid = threadIdx.x;
  const int sub = tid & (kSprLanes - 1);
  const int n = min(max(m.st->n, 0), p.kmax);
  const int nr = min(max(r.st->n, 0), r_kmax);
  const int i = blockIdx.x * (256 / kSprLanes) + tid / kSprLanes;
  int pre = spr::kNone;
  spr::Left L;
  L.x0 = 0;
  L.x1 = -1;
  L.yi = 0;
  if (i < n) {
    const float2 pos = m.pos[i], g = m.grad[i], rs = m.rs[i];
    pre = spr::left_setup(a, pos.x, pos.y, g.x, g.y, m.gnorm[i], rs.x, rs.y, &L);
  }
  spr::Fold f;
  spr::fold_clear(&f);
  if (pre < 0) {
    const int nrow = a.row_tol ? 3 : 1;
    for (int k = 0; k < nrow; ++k) {
      const int y = L.yi + (k == 0 ? 0 : (k == 1 ? -1 : 1));
      if (y < 0 || y >= a.rows) continue;
      const int* __restrict__ row = r.mask + (size_t)y * a.cols;
      for (int x = L.x0 + sub; x <= L.x1; x += kSprLanes) {
        const int j = row[x];
        if (j < 0 || j >= nr) continue;
        const float2 q = r.pos[j], h = r.grad[j];
        spr::fold_candidate(a, L, j, q.x, q.y, h.x, h.y, r.gnorm[j], &f);
      }
    }
  }
#pragma unroll
  for (int o = kSprLanes / 2; o > 0; o >>= 1) {
    spr::Fold t;
    t.seen = __shfl_xor(f.seen, o, kSprLanes);
    t.d_lo = __shfl_xor(f.d_lo, o, kSprLanes);
    t.d_hi = __shfl_xor(f.d_hi, o, kSprLanes);
    t.score = __shfl_xor(f.score, o, kSprLanes);
    t.d_win = __shfl_xor(f.d_win, o, kSprLanes);
    t.j = __shfl_xor(f.j, o, kSprLanes);
    spr::fold_join(&f, t);
  }
  int oc = pre, win = -1;
  const bool lead = sub == 0 && i < n;
  if (pre < 0) {
    oc = spr::decide(a, f);
    if (oc < 0) {
      float rho_n = 0.f, sig_n = 0.f;
      oc = spr::update(a, L, f.d_win, &rho_n, &sig_n);
      if ((oc & 7) == spr::kFused) {
        win = f.j;
        if (lead) m.rs[i] = make_float2(rho_n, sig_n);
      }
    }
  }
  if (sub == 0 && i < p.kmax) {
    outcome[i] = oc;
    winner[i] = win;
  }
  int nc[6];
  nc[0] = __popcll(__ballot(lead && oc != spr::kUnusable));
  nc[1] = __popcll(__ballot(lead && (f.seen & 1) != 0));
  nc[2] = __popcll(__ballot(lead && (oc & 7) == spr::kFused));
  nc[3] = __popcll(__ballot(lead && (oc & 7) == spr::kGated));
  nc[4] = __popcll(__ballot(lead && (oc & 7) == spr::kAmbiguous));
  nc[5] = __popcll(__ballot(lead && (oc & spr::kClampedBit) != 0));
  kf_add_counts(nc, sh_cnt, cnt + 1);
  if (blockIdx.x == 0 && tid == 0) cnt[0] = n;
}

void launch_stereo_prior(hipStream_t s, const KParams& p, const MapDev& m, const MapDev& r, int r_kmax, const spr::Args& a, int* cnt,
                         int* outcome, int* winner) {
  RH_LAUNCH(k_stereo_prior, dim3(div_up(p.kmax, 256 / kSprLanes)), dim3(256), 0, s, p, m, r, r_kmax, a, cnt, outcome, winner);
}

// ---- place recognition (rebvio_hip_map_place_signature, rebvio_hip_place_db_*) ---------------------------------------------------------
// place.hpp holds the definition's statements. Everything that crosses threads is an integer sum or a minimum of distinct keys,
// so no output word depends on an order.
//
// k_place_hist: one thread per keyline, the map's size read on the device. A workgroup fills a 384-word LDS histogram (+ the
// counted total as word 384) with LDS integer atomics and, behind a barrier, adds its non-zero words to hist[385] in global memory,
// which the caller cleared in front of the launch.
__global__ __launch_bounds__(256) void k_place_hist(KParams p, MapDev m, unsigned* __restrict__ hist) {
  __shared__ unsigned sh[plc::kWords + 1];
  const int tid = threadIdx.x;
  for (int k = tid; k <= plc::kWords; k += 256) sh[k] = 0u;
  __syncthreads();
  const int n = min(max(m.st->n, 0), p.kmax);
  const int i = blockIdx.x * 256 + tid;
  bool in = false;
  if (i < n) {
    const float2 pos = m.pos[i], g = m.grad[i];
    if (plc::counted(p.rows, p.cols, pos.x, pos.y, g.x, g.y, m.gnorm[i])) {
      in = true;
      atomicAdd(&sh[plc::word_of(p.rows, p.cols, pos.x, pos.y, g.x, g.y)], 1u);
    }
  }
  const int c = __popcll(__ballot(in));
  if ((tid & 63) == 0 && c) atomicAdd(&sh[plc::kWords], (unsigned)c);
  __syncthreads();
  for (int k = tid; k <= plc::kWords; k += 256) {
    const unsigned v = sh[k];
    if (v) atomicAdd(&hist[k], v);
  }
}

// k_place_norm: one workgroup. The 384 u16 words go straight to their destination (the context's query row, or a row of a
// database), the counted total next to its own.
__global__ __launch_bounds__(256) void k_place_norm(const unsigned* __restrict__ hist, uint16_t* __restrict__ sig, int* __restrict__ counted) {
  const unsigned n = hist[plc::kWords];
  for (int k = threadIdx.x; k < plc::kWords; k += 256) sig[k] = plc::normalise(hist[k], n);
  if (threadIdx.x == 0) *counted = (int)n;
}

// k_place_dist: one wave per database row. A row is 64 lanes x 12 bytes: lane l holds words 6l .. 6l + 5 as three dwords, the
// query's in registers for the wave's whole loop. Three sums of absolute differences of packed u16 pairs per lane and row
// (v_sad_u16), a butterfly over the wave, lane 0 stores dist[e]. A wave strides over the rows by the number of waves in the
// grid, kPlcUnroll rows at a time: their loads do not depend on each other and are in flight together.
struct PlcLane {
  unsigned a, b, c;
};
static_assert(sizeof(PlcLane) == 12 && alignof(PlcLane) == 4, "three dwords: one 12-byte load per lane");
__device__ __forceinline__ unsigned plc_lane_sad(const PlcLane& r, const PlcLane& q) {
  unsigned d = __builtin_amdgcn_sad_u16(r.a, q.a, 0u);
  d = __builtin_amdgcn_sad_u16(r.b, q.b, d);
  return __builtin_amdgcn_sad_u16(r.c, q.c, d);
}
__device__ __forceinline__ unsigned wave_sum_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
constexpr int kPlcUnroll = 4;
constexpr int kPlcDistBlocks = 2048;  // 8 workgroups of 4 waves per CU of an MI355X: every wave slot holds one
__global__ __launch_bounds__(256) void k_place_dist(const uint16_t* __restrict__ rows, int eligible, const uint16_t* __restrict__ query,
                                                    unsigned* __restrict__ dist) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int waves = gridDim.x * 4;
  const PlcLane q = reinterpret_cast<const PlcLane*>(query)[lane];
  const PlcLane* __restrict__ tab = reinterpret_cast<const PlcLane*>(rows);
  int e = wave;
  for (; e + (kPlcUnroll - 1) * waves < eligible; e += kPlcUnroll * waves) {
    PlcLane r[kPlcUnroll];
#pragma unroll
    for (int u = 0; u < kPlcUnroll; ++u) r[u] = tab[(size_t)(e + u * waves) * 64 + lane];
#pragma unroll
    for (int u = 0; u < kPlcUnroll; ++u) {
      const unsigned d = wave_sum_u(plc_lane_sad(r[u], q));
      if (lane == 0) dist[e + u * waves] = d;
    }
  }
  for (; e < eligible; e += waves) {
    const unsigned d = wave_sum_u(plc_lane_sad(tab[(size_t)e * 64 + lane], q));
    if (lane == 0) dist[e] = d;
  }
}

// k_place_topk: one workgroup of 1024. Keys are (dist << 32 | index) over the eligible rows, all distinct; min(k, eligible) rounds
// of "the smallest key above the previous winner". A thread keeps the smallest key of its own strided rows that has not won yet:
// one full scan in front of the rounds, and after a round only the winner's owner scans its rows again - every other thread's key
// is larger than the winner and stays what it was. Per round a butterfly on 64-bit minima inside each wave and LDS across the 16
// waves. res: the count (an int in a 16-byte head), then the records with tag 0 (the host owns the tags).
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)(v & 0xffffffffull), o), hi = __shfl_xor((unsigned)(v >> 32), o);
    const unsigned long long t = ((unsigned long long)hi << 32) | lo;
    v = t < v ? t : v;
  }
  return v;
}
// the smallest key >= lo among the rows tid, tid + 1024, ...: eight loads in flight at a time (the scan is a chain of L2 latencies)
__device__ __forceinline__ unsigned long long plc_scan(const unsigned* __restrict__ dist, int eligible, int tid, unsigned long long lo) {
  unsigned long long best = ~0ull;
  for (int e = tid; e < eligible; e += 8 * 1024) {
    unsigned d[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = e + u * 1024;
      d[u] = i < eligible ? dist[i] : 0u;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = e + u * 1024;
      const unsigned long long key = i < eligible ? ((unsigned long long)d[u] << 32) | (unsigned)i : ~0ull;
      if (key >= lo && key < best) best = key;
    }
  }
  return best;
}
__global__ __launch_bounds__(1024) void k_place_topk(const unsigned* __restrict__ dist, int eligible, int k, char* __restrict__ res) {
  __shared__ unsigned long long sh[16];
  __shared__ unsigned long long sh_win;
  const int tid = threadIdx.x;
  const int rounds = min(k, eligible);
  rebvio_hip_place_match* out = reinterpret_cast<rebvio_hip_place_match*>(res + 16);
  if (tid == 0) *reinterpret_cast<int*>(res) = rounds;
  unsigned long long mine = plc_scan(dist, eligible, tid, 0ull);
  for (int r = 0; r < rounds; ++r) {
    const unsigned long long best = wave_min_u64(mine);
    if ((tid & 63) == 0) sh[tid >> 6] = best;
    __syncthreads();
    if (tid < 64) {
      unsigned long long v = tid < 16 ? sh[tid] : ~0ull;
      v = wave_min_u64(v);
      if (tid == 0) {
        out[r].distance = (unsigned)(v >> 32);
        out[r].index = (int)(unsigned)(v & 0xffffffffull);
        out[r].tag = 0ull;
        sh_win = v;
      }
    }
    __syncthreads();
    const unsigned long long win = sh_win;
    if (((unsigned)(win & 0xffffffffull) & 1023u) == (unsigned)tid) mine = plc_scan(dist, eligible, tid, win + 1ull);
  }
}

void launch_place_signature(hipStream_t s, const KParams& p, const MapDev& m, unsigned* hist, uint16_t* sig, int* counted) {
  RH_LAUNCH(k_place_hist, dim3(div_up(p.kmax, 256)), dim3(256), 0, s, p, m, hist);
  RH_LAUNCH(k_place_norm, dim3(1), dim3(256), 0, s, hist, sig, counted);
}

void launch_place_query(hipStream_t s, const uint16_t* rows, int eligible, const uint16_t* query, int k, unsigned* dist, char* res) {
  const int blocks = div_up(eligible, 4) < kPlcDistBlocks ? div_up(eligible, 4) : kPlcDistBlocks;
  RH_LAUNCH(k_place_dist, dim3(blocks), dim3(256), 0, s, rows, eligible, query, dist);
  RH_LAUNCH(k_place_topk, dim3(1), dim3(1024), 0, s, dist, eligible, k, res);
}

}  // namespace rh
