// Stochastic-gradient MCMC: SGLD, SGHMC, SGNHT, contour SGLD (gfx950).  C ABI in include/bjx_hip.h ("SGMCMC").
//
// Reference: blackjax/sgmcmc/sgld.py, blackjax/sgmcmc/sghmc.py, blackjax/sgmcmc/sgnht.py, blackjax/sgmcmc/csgld.py
// (kernels), blackjax/sgmcmc/diffusions.py (overdamped_langevin, sghmc, sgnht),
// blackjax/util.py::generate_gaussian_noise.
//
// Layout and mapping: bjx_rows.h.  The gradient estimate comes from the user's callable (one autograd pass over a
// minibatch); everything else of a step is ONE launch here that draws its normals in registers.  Bytes per element:
//   bjx_sgld_step    r q, g          w q         12
//   bjx_sghmc_step   r q, p, g       w q, p      20   (first step, p drawn: 16; position-only last step: 12;
//                                                      both at once, num_integration_steps = 1: 8)
//   bjx_sgnht_step   r q, p, g       w q, p      20   (+ 8 B per chain for xi)
//   bjx_csgld_step   r q, g          w q         12   (+ 12 B per chain: the index and two histogram entries)
//   bjx_csgld_update r pdf           w pdf        8   per histogram entry (+ 12 B per chain: logdensity, pdf[i], index)
// The step kernels are bound by the RNG arithmetic of one normal per element (two in the first SGHMC step), as
// k_mala_propose is, so the operands are requested before it; k_csgld_update draws nothing and streams.
//
// VGPRs (kernel-resource-usage remark of the gfx950 build; 4-byte / 16-byte sweep), no scratch anywhere:
//   k_sgld_step 54 / 80 (k_mala_propose's figures), k_sghmc_step middle 62 / 100, first 62 / 112, last 38 / 46,
//   first + last 50 / 78, k_sgnht_step 63 / 94, k_csgld_step 70 / 95, k_csgld_update 90 / 98 (the fp64 pow).
#include <math.h>

#include "../../include/bjx_hip.h"
#include "bjx_device.h"
#include "bjx_host.h"
#include "bjx_rows.h"

using namespace bjx;

namespace {

// sgmcmc/diffusions.py::sghmc and ::sgnht share the noise scale sqrt(eps * T * (2 alpha - eps beta)), in fp32 in
// this order; NaN when 2 alpha < eps beta, as in the reference.
__device__ __forceinline__ float friction_noise_scale(float eps, float T, float alpha, float beta) {
  return sqrtf((eps * T) * (2.0f * alpha - eps * beta));
}

// sgmcmc/diffusions.py::overdamped_langevin (one_step): q1 = q + eps g + sqrt(2 T eps) normal(chain key, (D,)),
// left to right, each `x + s * y` one fmaf.  sgmcmc/sgld.py hands the chain key to the diffusion unsplit.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_sgld_step(Key key, int64_t off, int64_t fold, int64_t N, int64_t D, float eps_s, const float* __restrict__ eps_pc,
            float T_s, const float* __restrict__ T_pc, const float* __restrict__ q, const float* __restrict__ g,
            float* __restrict__ q_out) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = wave_row0(); r < N; r += wave_row_stride()) {
    const Key kc = chain_key(key, (uint64_t)(r + off), fold);
    const float eps = eps_pc ? eps_pc[r] : eps_s;
    const float T = T_pc ? T_pc[r] : T_s;
    const float s = sqrtf((2.0f * T) * eps);
    const int64_t base = r * D;
    for (int64_t j = (int64_t)lane * VEC; j < D; j += 64 * VEC) {
      float qq[VEC], gg[VEC], z[VEC], qn[VEC];
      ldv<VEC>(q + base + j, qq);
      ldv<VEC>(g + base + j, gg);
      normalv<VEC>(kc, j, z);
#pragma unroll
      for (int e = 0; e < VEC; ++e) qn[e] = fmaf(s, z[e], fmaf(eps, gg[e], qq[e]));
      stv<VEC>(q_out + base + j, qn);
    }
  }
}

// Integration step `l` of sgmcmc/sghmc.py (kernel) with sgmcmc/diffusions.py::sghmc:
//   q_{l+1} = q_l + eps p_l ; p_{l+1} = (1 - alpha eps) p_l + eps g_l + s normal(split(chain key, L)[l], (D,)).
// DRAW: p_l is the momentum refresh normal(chain key, (D,)) itself (l = 0), drawn here instead of read.
// POS_ONLY: only q_{l+1} is written (l = L - 1: the reference drops the final momentum, so neither the gradient nor
// the noise of that step is needed).
template <int VEC, bool DRAW, bool POS_ONLY>
__global__ void __launch_bounds__(kBlock)
k_sghmc_step(Key key, int64_t off, int64_t fold, int64_t N, int64_t D, int64_t step_index, float alpha, float beta,
             float eps_s, const float* __restrict__ eps_pc, float T_s, const float* __restrict__ T_pc,
             const float* __restrict__ q, const float* __restrict__ p_in, const float* __restrict__ g,
             float* __restrict__ q_out, float* __restrict__ p_out) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = wave_row0(); r < N; r += wave_row_stride()) {
    const Key kc = chain_key(key, (uint64_t)(r + off), fold);
    const Key kn = key_child(kc, (uint64_t)step_index);
    const float eps = eps_pc ? eps_pc[r] : eps_s;
    const float T = T_pc ? T_pc[r] : T_s;
    const float c = 1.0f - alpha * eps;  // two fp32 roundings
    const float s = friction_noise_scale(eps, T, alpha, beta);
    const int64_t base = r * D;
    for (int64_t j = (int64_t)lane * VEC; j < D; j += 64 * VEC) {
      float qq[VEC], pp[VEC], gg[VEC], z[VEC], qn[VEC], pn[VEC];
      ldv<VEC>(q + base + j, qq);
      if constexpr (!DRAW) ldv<VEC>(p_in + base + j, pp);
      if constexpr (!POS_ONLY) ldv<VEC>(g + base + j, gg);
      if constexpr (DRAW) normalv<VEC>(kc, j, pp);
#pragma unroll
      for (int e = 0; e < VEC; ++e) qn[e] = fmaf(eps, pp[e], qq[e]);
      stv<VEC>(q_out + base + j, qn);
      if constexpr (!POS_ONLY) {
        normalv<VEC>(kn, j, z);
#pragma unroll
        for (int e = 0; e < VEC; ++e) pn[e] = fmaf(s, z[e], fmaf(eps, gg[e], c * pp[e]));
        stv<VEC>(p_out + base + j, pn);
      }
    }
  }
}

// sgmcmc/diffusions.py::sgnht (one_step), noise normal(chain key, (D,)) (sgmcmc/sgnht.py hands the key on unsplit):
//   q1 = q + eps p ; p1 = p - (eps xi) p + eps g + s z ; xi1 = xi + eps (mean_j p1_j^2 - T)
// One pass: the sum of squares accumulates in fp64 per lane while p1 is stored, then wave_sum; every lane computes
// xi1 and lane 0 writes it.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_sgnht_step(Key key, int64_t off, int64_t fold, int64_t N, int64_t D, float alpha, float beta, float eps_s,
             const float* __restrict__ eps_pc, float T_s, const float* __restrict__ T_pc,
             const float* __restrict__ q, const float* __restrict__ p, const float* __restrict__ xi,
             const float* __restrict__ g, float* __restrict__ q_out, float* __restrict__ p_out,
             float* __restrict__ xi_out) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = wave_row0(); r < N; r += wave_row_stride()) {
    const Key kc = chain_key(key, (uint64_t)(r + off), fold);
    const float eps = eps_pc ? eps_pc[r] : eps_s;
    const float T = T_pc ? T_pc[r] : T_s;
    const float x = xi[r];
    const float nex = -(eps * x);
    const float s = friction_noise_scale(eps, T, alpha, beta);
    const int64_t base = r * D;
    double acc = 0.0;
    for (int64_t j = (int64_t)lane * VEC; j < D; j += 64 * VEC) {
      float qq[VEC], pp[VEC], gg[VEC], z[VEC], qn[VEC], pn[VEC];
      ldv<VEC>(q + base + j, qq);
      ldv<VEC>(p + base + j, pp);
      ldv<VEC>(g + base + j, gg);
      normalv<VEC>(kc, j, z);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        qn[e] = fmaf(eps, pp[e], qq[e]);
        pn[e] = fmaf(s, z[e], fmaf(eps, gg[e], fmaf(nex, pp[e], pp[e])));
        acc += (double)pn[e] * (double)pn[e];
      }
      stv<VEC>(q_out + base + j, qn);
      stv<VEC>(p_out + base + j, pn);
    }
    acc = wave_sum(acc);
    const float m = (float)(acc / (double)D);
    const float x1 = fmaf(eps, m - T, x);
    if (lane == 0) xi_out[r] = x1;
  }
}

// sgmcmc/csgld.py (kernel), the position half: overdamped_langevin on the gradient scaled by
//   m = 1 + zeta T (log pdf[i] - log pdf[i - 1]) / energy_gap,  i = the chain's energy index,
// the slope of the chain's own energy histogram.  m is wave-uniform: both logs in fp64 rounded once, then fp32 in
// the order written; `m * g` is rounded before the fma, so the scaled gradient exists only in registers.  The index
// is clamped into [1, M - 1] on read: no state can make the histogram loads leave the row.
template <int VEC>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(5)))  // 4 waves without it (99 VGPRs)
k_csgld_step(Key key, int64_t off, int64_t fold, int64_t N, int64_t D, int64_t M, float zeta, float gap, float eps_s,
             const float* __restrict__ eps_pc, float T_s, const float* __restrict__ T_pc, const float* __restrict__ q,
             const float* __restrict__ g, const float* __restrict__ pdf, const int32_t* __restrict__ idx,
             float* __restrict__ q_out) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = wave_row0(); r < N; r += wave_row_stride()) {
    const Key kc = chain_key(key, (uint64_t)(r + off), fold);
    const float eps = eps_pc ? eps_pc[r] : eps_s;
    const float T = T_pc ? T_pc[r] : T_s;
    const float s = sqrtf((2.0f * T) * eps);
    int64_t i = (int64_t)idx[r];
    i = i < 1 ? 1 : (i > M - 1 ? M - 1 : i);
    // one fp64 log per row instead of two: even lanes take pdf[i], odd lanes pdf[i - 1]; lanes 0 and 1 hand them on
    const int ll = __builtin_bit_cast(int, (float)log((double)pdf[r * M + i - (lane & 1)]));
    const float la = __builtin_bit_cast(float, __builtin_amdgcn_readlane(ll, 0));
    const float lb = __builtin_bit_cast(float, __builtin_amdgcn_readlane(ll, 1));
    const float m = 1.0f + (((zeta * T) * (la - lb)) / gap);
    const int64_t base = r * D;
    for (int64_t j = (int64_t)lane * VEC; j < D; j += 64 * VEC) {
      float qq[VEC], gg[VEC], z[VEC], qn[VEC];
      ldv<VEC>(q + base + j, qq);
      ldv<VEC>(g + base + j, gg);
      normalv<VEC>(kc, j, z);
#pragma unroll
      for (int e = 0; e < VEC; ++e) qn[e] = fmaf(s, z[e], fmaf(eps, m * gg[e], qq[e]));
      stv<VEC>(q_out + base + j, qn);
    }
  }
}

// sgmcmc/csgld.py (kernel), the histogram half, from the log-density estimate at the NEW position:
//   i = clamp(floor((-logdensity - min_energy) / energy_gap + 1), 1, M - 1)
//   pdf_out = pdf + (eps_sa pdf[i]^zeta) (e_i - pdf),  pdf[i] of the OLD histogram
// The clamp is in floating point, before the conversion: NaN -> 1 (the reference's NaN -> 0 conversion, then its
// clamp), -inf energy -> 1, +inf energy -> M - 1.  pow in fp64 rounded once; zeta == 1 skips it.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_csgld_update(int64_t N, int64_t M, float zeta, float gap, float min_energy, float eps_s,
               const float* __restrict__ eps_pc, const float* __restrict__ logdensity,
               const float* __restrict__ pdf_in, float* __restrict__ pdf_out, int32_t* __restrict__ idx_out) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = wave_row0(); r < N; r += wave_row_stride()) {
    const float eps = eps_pc ? eps_pc[r] : eps_s;
    const float x = floorf(((-logdensity[r] - min_energy) / gap) + 1.0f);
    const float top = (float)(M - 1);
    const int64_t i = !(x >= 1.0f) ? 1 : (x >= top ? M - 1 : (int64_t)x);
    const int64_t base = r * M;
    const float a = pdf_in[base + i];
    const float w = eps * (zeta == 1.0f ? a : (float)pow((double)a, (double)zeta));
    for (int64_t j = (int64_t)lane * VEC; j < M; j += 64 * VEC) {
      float pp[VEC], pn[VEC];
      ldv<VEC>(pdf_in + base + j, pp);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const float u = (j + e == i) ? 1.0f - pp[e] : -pp[e];
        pn[e] = fmaf(w, u, pp[e]);
      }
      stv<VEC>(pdf_out + base + j, pn);
    }
    if (lane == 0) idx_out[r] = (int32_t)i;
  }
}

}  // namespace

extern "C" {

int bjx_sgld_step(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold, int64_t N,
                  int64_t D, float eps, const float* eps_per_chain, float temperature,
                  const float* temperature_per_chain, const float* q, const float* g, float* q_out) {
  BJX_CHECK_ARG(N >= 0 && D > 0, "bjx_sgld_step: bad sizes");
  if (N == 0) return 0;
  BJX_CHECK_ARG(q && g && q_out, "bjx_sgld_step: null pointer");
  BJX_LAUNCH_ROWS_VEC(bjx_vec4_ok(D, q, g, q_out), k_sgld_step, N, stream, Key{key0, key1}, chain_offset, step_fold,
                      N, D, eps, eps_per_chain, temperature, temperature_per_chain, q, g, q_out);
  return bjx_check_launch("bjx_sgld_step");
}

int bjx_sghmc_step(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold, int64_t N,
                   int64_t D, int64_t step_index, float alpha, float beta, float eps, const float* eps_per_chain,
                   float temperature, const float* temperature_per_chain, const float* q, const float* p_in,
                   const float* g, float* q_out, float* p_out) {
  BJX_CHECK_ARG(N >= 0 && D > 0 && step_index >= 0, "bjx_sghmc_step: bad sizes");
  if (N == 0) return 0;
  BJX_CHECK_ARG(q && q_out, "bjx_sghmc_step: null pointer");
  BJX_CHECK_ARG((g == nullptr) == (p_out == nullptr),
                "bjx_sghmc_step: g and p_out must both be given, or both be null (position-only last step)");
  const bool v4 = bjx_vec4_ok(D, q, p_in, g, q_out, p_out);
#define BJX_SGHMC_STEP(DRAW, POS_ONLY)                                                                            \
  do {                                                                                                            \
    if (v4)                                                                                                       \
      BJX_LAUNCH_ROWS((k_sghmc_step<4, DRAW, POS_ONLY>), N, stream, Key{key0, key1}, chain_offset, step_fold, N,  \
                      D, step_index, alpha, beta, eps, eps_per_chain, temperature, temperature_per_chain, q, p_in, \
                      g, q_out, p_out);                                                                           \
    else                                                                                                          \
      BJX_LAUNCH_ROWS((k_sghmc_step<1, DRAW, POS_ONLY>), N, stream, Key{key0, key1}, chain_offset, step_fold, N,  \
                      D, step_index, alpha, beta, eps, eps_per_chain, temperature, temperature_per_chain, q, p_in, \
                      g, q_out, p_out);                                                                           \
  } while (0)
  if (p_in == nullptr) {
    if (g == nullptr) BJX_SGHMC_STEP(true, true);
    else BJX_SGHMC_STEP(true, false);
  } else {
    if (g == nullptr) BJX_SGHMC_STEP(false, true);
    else BJX_SGHMC_STEP(false, false);
  }
#undef BJX_SGHMC_STEP
  return bjx_check_launch("bjx_sghmc_step");
}

int bjx_sgnht_step(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold, int64_t N,
                   int64_t D, float alpha, float beta, float eps, const float* eps_per_chain, float temperature,
                   const float* temperature_per_chain, const float* q, const float* p, const float* xi,
                   const float* g, float* q_out, float* p_out, float* xi_out) {
  BJX_CHECK_ARG(N >= 0 && D > 0, "bjx_sgnht_step: bad sizes");
  if (N == 0) return 0;
  BJX_CHECK_ARG(q && p && xi && g && q_out && p_out && xi_out, "bjx_sgnht_step: null pointer");
  BJX_LAUNCH_ROWS_VEC(bjx_vec4_ok(D, q, p, g, q_out, p_out), k_sgnht_step, N, stream, Key{key0, key1}, chain_offset,
                      step_fold, N, D, alpha, beta, eps, eps_per_chain, temperature, temperature_per_chain, q, p, xi,
                      g, q_out, p_out, xi_out);
  return bjx_check_launch("bjx_sgnht_step");
}

int bjx_csgld_step(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold, int64_t N,
                   int64_t D, int64_t M, float zeta, float energy_gap, float eps, const float* eps_per_chain,
                   float temperature, const float* temperature_per_chain, const float* q, const float* g,
                   const float* energy_pdf, const int32_t* energy_idx, float* q_out) {
  BJX_CHECK_ARG(N >= 0 && D > 0 && M >= 2 && M <= INT32_MAX, "bjx_csgld_step: bad sizes");
  if (N == 0) return 0;
  BJX_CHECK_ARG(q && g && energy_pdf && energy_idx && q_out, "bjx_csgld_step: null pointer");
  BJX_LAUNCH_ROWS_VEC(bjx_vec4_ok(D, q, g, q_out), k_csgld_step, N, stream, Key{key0, key1}, chain_offset, step_fold,
                      N, D, M, zeta, energy_gap, eps, eps_per_chain, temperature, temperature_per_chain, q, g,
                      energy_pdf, energy_idx, q_out);
  return bjx_check_launch("bjx_csgld_step");
}

int bjx_csgld_update(void* stream, int64_t N, int64_t M, float zeta, float energy_gap, float min_energy, float eps_sa,
                     const float* eps_sa_per_chain, const float* logdensity, const float* pdf_in, float* pdf_out,
                     int32_t* idx_out) {
  BJX_CHECK_ARG(N >= 0 && M >= 2 && M <= INT32_MAX, "bjx_csgld_update: bad sizes");
  if (N == 0) return 0;
  BJX_CHECK_ARG(logdensity && pdf_in && pdf_out && idx_out, "bjx_csgld_update: null pointer");
  BJX_LAUNCH_ROWS_VEC(bjx_vec4_ok(M, pdf_in, pdf_out), k_csgld_update, N, stream, N, M, zeta, energy_gap, min_energy,
                      eps_sa, eps_sa_per_chain, logdensity, pdf_in, pdf_out, idx_out);
  return bjx_check_launch("bjx_csgld_update");
}

}  // extern "C"
