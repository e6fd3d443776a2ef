// Barker proposal sampler (gfx950).  C ABI in include/bjx_hip.h ("Barker").
//
// Reference: blackjax/mcmc/barker.py (init, build_kernel: _barker_sample_nd, _barker_logpdf, kernel) with a
// diagonal preconditioner, mcmc/proposal.py::compute_asymmetric_acceptance_ratio, static_binomial_sampling,
// safe_energy_diff.  Livingstone & Zanella 2022.
//
// Layout and mapping: bjx_rows.h.  A transition is propose -> user callable -> finish:
// 12 (16 with a per-chain metric) + 8 + 24 bytes per element.
#include <math.h>

#include "../../include/bjx_hip.h"
#include "bjx_device.h"
#include "bjx_host.h"
#include "bjx_rows.h"

using namespace bjx;

namespace {

// jax.scipy.special.expit in fp64, rounded once to fp32 (the oracle's expit_cr)
__device__ __forceinline__ float expit_cr(float x) { return (float)(1.0 / (1.0 + exp(-(double)x))); }

// softplus(x) = max(x, 0) + log1p(exp(-|x|)) in fp64.  A NaN x gives NaN through the second term.
__device__ __forceinline__ double softplus64(float x) {
  const double xd = (double)x;
  return fmax(xd, 0.0) + log1p(exp(-fabs(xd)));
}

// barker.py::_barker_sample_nd with a diagonal scale: per element
//   z = (tau * sqrt(imm)) * normal(k1, (D,)) ; p = expit(z * g0) ; b = uniform(k2, (D,)) < p ; q1 = q0 +- z
// with k1, k2 = split(split(chain key, 2)[0], 2).  A NaN p compares false: the element takes q0 - z.
// Reads q0, g0 (and a per-chain imm row), writes q1: 12 / 16 B per element.  Two threefry blocks, one erf_inv and
// one fp64 expit per element: bound by that arithmetic, not by HBM (DESIGN.md kernel table).
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_barker_propose(Key key, int64_t off, int64_t fold, int64_t N, int64_t D, float tau_s,
                 const float* __restrict__ tau_pc, const float* __restrict__ imm, int64_t imm_stride,
                 const float* __restrict__ q0, const float* __restrict__ g0, float* __restrict__ q1_out) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = wave_row0(); r < N; r += wave_row_stride()) {
    const Key kc = chain_key(key, (uint64_t)(r + off), fold);
    const Key ks = key_child(kc, 0);  // key_sample, key_rmh = split(rng_key)
    const Key kn = key_child(ks, 0), ku = key_child(ks, 1);
    const float tau = tau_pc ? tau_pc[r] : tau_s;
    const int64_t base = r * D;
    const float* im = imm ? imm + r * imm_stride : nullptr;
    for (int64_t j = (int64_t)lane * VEC; j < D; j += 64 * VEC) {
      float qq[VEC], gg[VEC], mm[VEC], n[VEC], qn[VEC];
      ldv<VEC>(q0 + base + j, qq);
      ldv<VEC>(g0 + base + j, gg);
      if (im) {
        ldv<VEC>(im + j, mm);
      } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) mm[e] = 1.0f;
      }
      normalv<VEC>(kn, j, n);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const float u = unit_float(key_bits32(ku, (uint64_t)(j + e)));  // uniform(k2, (D,))[j + e]
        const float s = tau * sqrtf(mm[e]);
        const float z = s * n[e];
        const float p = expit_cr(z * gg[e]);
        qn[e] = (u < p) ? qq[e] + z : qq[e] - z;
      }
      stv<VEC>(q1_out + base + j, qn);
    }
  }
}

// One element's contribution to log q(x | y) - log q(y | x) = sum softplus(-(y - x) g_x) - softplus((y - x) g_y)
// (barker.py::_barker_logpdf both ways; the diagonal scale cancels inside the products).
__device__ __forceinline__ double barker_term(float a0, float a1, float b0, float b1) {
  const float t = a1 - a0;
  const float a = -(t * b0);
  const float e = t * b1;
  return softplus64(a) - softplus64(e);
}

// The per-chain scalar tail (every lane computes it; lane 0 writes): metropolis_accept on safe_energy_diff of the
// log ratio, key_rmh = split(chain key, 2)[1].
__device__ __forceinline__ bool barker_accept(Key key, int64_t gidx, int64_t fold, double sum, float lp0,
                                              float lp1, float* p_acc_out) {
  const float log_ratio = (lp1 - lp0) + (float)sum;
  return metropolis_accept(key, gidx, fold, safe_energy_diff(log_ratio), p_acc_out);
}

// General two-pass finish.  Pass 1 sweeps q0, q1, g0, g1 once and accumulates the fp64 sum; pass 2 copies the
// accepted or the kept state (wave-uniform source rows) out of place.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_barker_finish(Key key, int64_t off, int64_t fold, int64_t N, int64_t D, const float* __restrict__ q0,
                const float* __restrict__ logp0, const float* __restrict__ g0, const float* __restrict__ q1,
                const float* __restrict__ logp1, const float* __restrict__ g1, float* __restrict__ q_out,
                float* __restrict__ logp_out, float* __restrict__ g_out, float* __restrict__ acc_rate_out,
                uint8_t* __restrict__ is_acc_out) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = wave_row0(); r < N; r += wave_row_stride()) {
    const int64_t base = r * D;
    double acc = 0.0;
    for (int64_t j = (int64_t)lane * VEC; j < D; j += 64 * VEC) {
      float a0[VEC], a1[VEC], b0[VEC], b1[VEC];
      ldv<VEC>(q0 + base + j, a0);
      ldv<VEC>(q1 + base + j, a1);
      ldv<VEC>(g0 + base + j, b0);
      ldv<VEC>(g1 + base + j, b1);
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc += barker_term(a0[e], a1[e], b0[e], b1[e]);
    }
    acc = wave_sum(acc);
    const float lp0 = logp0[r], lp1 = logp1[r];
    float p_acc;
    const bool accept = barker_accept(key, r + off, fold, acc, lp0, lp1, &p_acc);
    if (lane == 0) {
      acc_rate_out[r] = p_acc;
      is_acc_out[r] = accept ? 1 : 0;
      logp_out[r] = accept ? lp1 : lp0;
    }
    const float* qs = accept ? q1 : q0;
    const float* gs = accept ? g1 : g0;
    for (int64_t j = (int64_t)lane * VEC; j < D; j += 64 * VEC) {
      float a[VEC], b[VEC];
      ldv<VEC>(qs + base + j, a);
      ldv<VEC>(gs + base + j, b);
      stv<VEC>(q_out + base + j, a);
      stv<VEC>(g_out + base + j, b);
    }
  }
}

// The same for 16-byte rows of at most 256 * NI floats: all four operands stay in registers between the
// reduction and the select, so the launch moves 16 B read + 8 B written per element and re-reads nothing.
template <int NI>
__global__ void __launch_bounds__(kBlock)
k_barker_finish_res(Key key, int64_t off, int64_t fold, int64_t N, int64_t D, const float* __restrict__ q0,
                    const float* __restrict__ logp0, const float* __restrict__ g0, const float* __restrict__ q1,
                    const float* __restrict__ logp1, const float* __restrict__ g1, float* __restrict__ q_out,
                    float* __restrict__ logp_out, float* __restrict__ g_out, float* __restrict__ acc_rate_out,
                    uint8_t* __restrict__ is_acc_out) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = wave_row0(); r < N; r += wave_row_stride()) {
    const int64_t base = r * D;
    F4 Q0[NI], Q1[NI], G0[NI], G1[NI];
    bool ok[NI];
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      const int64_t j = ((int64_t)lane + 64 * k) * 4;
      ok[k] = j < D;
      if (ok[k]) {
        Q0[k] = ld4(q0 + base + j);
        Q1[k] = ld4(q1 + base + j);
        G0[k] = ld4(g0 + base + j);
        G1[k] = ld4(g1 + base + j);
      }
    }
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < NI; ++k)
      if (ok[k]) {
        const float a0[4] = {Q0[k].x, Q0[k].y, Q0[k].z, Q0[k].w}, a1[4] = {Q1[k].x, Q1[k].y, Q1[k].z, Q1[k].w};
        const float b0[4] = {G0[k].x, G0[k].y, G0[k].z, G0[k].w}, b1[4] = {G1[k].x, G1[k].y, G1[k].z, G1[k].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) acc += barker_term(a0[e], a1[e], b0[e], b1[e]);
      }
    acc = wave_sum(acc);
    const float lp0 = logp0[r], lp1 = logp1[r];
    float p_acc;
    const bool accept = barker_accept(key, r + off, fold, acc, lp0, lp1, &p_acc);
    if (lane == 0) {
      acc_rate_out[r] = p_acc;
      is_acc_out[r] = accept ? 1 : 0;
      logp_out[r] = accept ? lp1 : lp0;
    }
#pragma unroll
    for (int k = 0; k < NI; ++k)
      if (ok[k]) {
        const int64_t j = ((int64_t)lane + 64 * k) * 4;
        st4(q_out + base + j, accept ? Q1[k] : Q0[k]);
        st4(g_out + base + j, accept ? G1[k] : G0[k]);
      }
  }
}

}  // namespace

extern "C" {

int bjx_barker_propose(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold,
                       int64_t N, int64_t D, float tau, const float* tau_per_chain, const float* imm,
                       int64_t imm_row_stride, const float* q0, const float* g0, float* q1_out) {
  BJX_CHECK_ARG(N >= 0 && D > 0, "bjx_barker_propose: bad sizes");
  if (N == 0) return 0;
  BJX_CHECK_ARG(q0 && g0 && q1_out, "bjx_barker_propose: null pointer");
  BJX_CHECK_ARG(!imm || imm_row_stride == 0 || imm_row_stride == D, "bjx_barker_propose: bad imm stride");
  BJX_LAUNCH_ROWS_VEC(bjx_vec4_ok(D, q0, g0, q1_out, imm), k_barker_propose, N, stream, Key{key0, key1},
                      chain_offset, step_fold, N, D, tau, tau_per_chain, imm, imm_row_stride, q0, g0, q1_out);
  return bjx_check_launch("bjx_barker_propose");
}

int bjx_barker_finish(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold,
                      int64_t N, int64_t D, const float* q0, const float* logp0, const float* g0,
                      const float* q1, const float* logp1, const float* g1, float* q_out, float* logp_out,
                      float* g_out, float* acceptance_rate_out, uint8_t* is_accepted_out) {
  BJX_CHECK_ARG(N >= 0 && D > 0, "bjx_barker_finish: bad sizes");
  if (N == 0) return 0;
  BJX_CHECK_ARG(q0 && logp0 && g0 && q1 && logp1 && g1 && q_out && logp_out && g_out && acceptance_rate_out &&
                    is_accepted_out,
                "bjx_barker_finish: null pointer");
#define BJX_BARKER_FINISH(KERNEL)                                                                          \
  BJX_LAUNCH_ROWS(KERNEL, N, stream, Key{key0, key1}, chain_offset, step_fold, N, D, q0, logp0, g0, q1, logp1, \
                  g1, q_out, logp_out, g_out, acceptance_rate_out, is_accepted_out)
  if (bjx_vec4_ok(D, q0, g0, q1, g1, q_out, g_out)) {
    if (D <= 256) BJX_BARKER_FINISH(k_barker_finish_res<1>);
    else if (D <= 512) BJX_BARKER_FINISH(k_barker_finish_res<2>);
    else if (D <= 1024) BJX_BARKER_FINISH(k_barker_finish_res<4>);
    else BJX_BARKER_FINISH(k_barker_finish<4>);
  } else {
    BJX_BARKER_FINISH(k_barker_finish<1>);
  }
#undef BJX_BARKER_FINISH
  return bjx_check_launch("bjx_barker_finish");
}

}  // extern "C"
