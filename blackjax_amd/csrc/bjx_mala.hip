// Metropolis-adjusted Langevin algorithm (gfx950).  C ABI in include/bjx_hip.h ("MALA").
//
// Reference: blackjax/mcmc/mala.py (init, build_kernel: transition_energy, kernel),
// mcmc/diffusions.py::overdamped_langevin, mcmc/proposal.py::compute_asymmetric_acceptance_ratio,
// static_binomial_sampling, safe_energy_diff.
//
// Layout and mapping: bjx_rows.h.  A transition is propose -> user callable -> finish: 12 + 8 + 24 = 44 bytes
// per element.
#include <math.h>

#include "../../include/bjx_hip.h"
#include "bjx_device.h"
#include "bjx_host.h"
#include "bjx_rows.h"

using namespace bjx;

namespace {

// diffusions.py::overdamped_langevin (one_step): q1 = q0 + tau * g0 + sqrt(2 tau) * normal(key_integrator, (D,)),
// left to right, each `x + s * y` one fmaf.  key_integrator = split(chain key, 2)[0] (mala.py kernel).
// Reads q0, g0, writes q1 (12 B per element); bound by the RNG arithmetic of one normal per element
// (threefry + erf_inv), as k_momentum_diag is -- the two operands are requested before it.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_mala_propose(Key key, int64_t off, int64_t fold, int64_t N, int64_t D, float tau_s,
               const float* __restrict__ tau_pc, const float* __restrict__ q0, const float* __restrict__ g0,
               float* __restrict__ q1_out) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = wave_row0(); r < N; r += wave_row_stride()) {
    const Key kc = chain_key(key, (uint64_t)(r + off), fold);
    const Key kn = key_child(kc, 0);  // key_integrator, key_rmh = split(rng_key)
    const float tau = tau_pc ? tau_pc[r] : tau_s;
    const float s = sqrtf(2.0f * tau);
    const int64_t base = r * D;
    for (int64_t j = (int64_t)lane * VEC; j < D; j += 64 * VEC) {
      float qq[VEC], gg[VEC], z[VEC], qn[VEC];
      ldv<VEC>(q0 + base + j, qq);
      ldv<VEC>(g0 + base + j, gg);
      normalv<VEC>(kn, j, z);
#pragma unroll
      for (int e = 0; e < VEC; ++e) qn[e] = fmaf(s, z[e], fmaf(tau, gg[e], qq[e]));
      stv<VEC>(q1_out + base + j, qn);
    }
  }
}

// The per-chain scalar tail of a transition, from the two fp64 sums of squares (every lane computes it; lane 0
// writes).  mala.py transition_energy: -logp(new) + 0.25 * (1 / tau) * sum theta^2 with
// theta = state.position - new.position - tau * new.grad; metropolis_accept on
// safe_energy_diff(E(new, state), E(state, new)), key_rmh = split(chain key, 2)[1].
__device__ __forceinline__ bool mala_accept(Key key, int64_t gidx, int64_t fold, float tau, double sum_new,
                                            double sum_prev, float lp0, float lp1, float* p_acc_out) {
  const float c = 0.25f * (1.0f / tau);  // two fp32 roundings, as written in mala.py
  const float e_new = fmaf(c, (float)sum_new, -lp1);    // transition_energy(state, new_state)
  const float e_prev = fmaf(c, (float)sum_prev, -lp0);  // transition_energy(new_state, state)
  return metropolis_accept(key, gidx, fold, safe_energy_diff(e_prev - e_new), p_acc_out);
}

// General two-pass finish.  Pass 1 sweeps q0, q1, g0, g1 once and accumulates both sums of squares; pass 2
// copies the accepted or the kept state (wave-uniform source rows) out of place.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_mala_finish(Key key, int64_t off, int64_t fold, int64_t N, int64_t D, float tau_s,
              const float* __restrict__ tau_pc, const float* __restrict__ q0, const float* __restrict__ logp0,
              const float* __restrict__ g0, const float* __restrict__ q1, const float* __restrict__ logp1,
              const float* __restrict__ g1, float* __restrict__ q_out, float* __restrict__ logp_out,
              float* __restrict__ g_out, float* __restrict__ acc_rate_out, uint8_t* __restrict__ is_acc_out) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = wave_row0(); r < N; r += wave_row_stride()) {
    const float tau = tau_pc ? tau_pc[r] : tau_s;
    const float ntau = -tau;
    const int64_t base = r * D;
    double acc_new = 0.0, acc_prev = 0.0;
    for (int64_t j = (int64_t)lane * VEC; j < D; j += 64 * VEC) {
      float a0[VEC], a1[VEC], b0[VEC], b1[VEC];
      ldv<VEC>(q0 + base + j, a0);
      ldv<VEC>(q1 + base + j, a1);
      ldv<VEC>(g0 + base + j, b0);
      ldv<VEC>(g1 + base + j, b1);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const float tn = fmaf(ntau, b1[e], a0[e] - a1[e]);
        const float tp = fmaf(ntau, b0[e], a1[e] - a0[e]);
        acc_new += (double)tn * (double)tn;
        acc_prev += (double)tp * (double)tp;
      }
    }
    acc_new = wave_sum(acc_new);
    acc_prev = wave_sum(acc_prev);
    const float lp0 = logp0[r], lp1 = logp1[r];
    float p_acc;
    const bool accept = mala_accept(key, r + off, fold, tau, acc_new, acc_prev, lp0, lp1, &p_acc);
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
// NI = 1 / 2 / 4: 66 / 71 / 105 VGPRs, no scratch (kernel-resource-usage remark of the gfx950 build; the two-pass
// kernel, which holds no row, takes 62 / 70 for its 4-byte / 16-byte sweep).
template <int NI>
__global__ void __launch_bounds__(kBlock)
k_mala_finish_res(Key key, int64_t off, int64_t fold, int64_t N, int64_t D, float tau_s,
                  const float* __restrict__ tau_pc, const float* __restrict__ q0,
                  const float* __restrict__ logp0, const float* __restrict__ g0, const float* __restrict__ q1,
                  const float* __restrict__ logp1, const float* __restrict__ g1, float* __restrict__ q_out,
                  float* __restrict__ logp_out, float* __restrict__ g_out, float* __restrict__ acc_rate_out,
                  uint8_t* __restrict__ is_acc_out) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = wave_row0(); r < N; r += wave_row_stride()) {
    const float tau = tau_pc ? tau_pc[r] : tau_s;
    const float ntau = -tau;
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
    double acc_new = 0.0, acc_prev = 0.0;
#pragma unroll
    for (int k = 0; k < NI; ++k)
      if (ok[k]) {
        const float a0[4] = {Q0[k].x, Q0[k].y, Q0[k].z, Q0[k].w}, a1[4] = {Q1[k].x, Q1[k].y, Q1[k].z, Q1[k].w};
        const float b0[4] = {G0[k].x, G0[k].y, G0[k].z, G0[k].w}, b1[4] = {G1[k].x, G1[k].y, G1[k].z, G1[k].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float tn = fmaf(ntau, b1[e], a0[e] - a1[e]);
          const float tp = fmaf(ntau, b0[e], a1[e] - a0[e]);
          acc_new += (double)tn * (double)tn;
          acc_prev += (double)tp * (double)tp;
        }
      }
    acc_new = wave_sum(acc_new);
    acc_prev = wave_sum(acc_prev);
    const float lp0 = logp0[r], lp1 = logp1[r];
    float p_acc;
    const bool accept = mala_accept(key, r + off, fold, tau, acc_new, acc_prev, lp0, lp1, &p_acc);
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

int bjx_mala_propose(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold,
                     int64_t N, int64_t D, float tau, const float* tau_per_chain, const float* q0,
                     const float* g0, float* q1_out) {
  BJX_CHECK_ARG(N >= 0 && D > 0, "bjx_mala_propose: bad sizes");
  if (N == 0) return 0;
  BJX_CHECK_ARG(q0 && g0 && q1_out, "bjx_mala_propose: null pointer");
  BJX_LAUNCH_ROWS_VEC(bjx_vec4_ok(D, q0, g0, q1_out), k_mala_propose, N, stream, Key{key0, key1}, chain_offset,
                      step_fold, N, D, tau, tau_per_chain, q0, g0, q1_out);
  return bjx_check_launch("bjx_mala_propose");
}

int bjx_mala_finish(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold,
                    int64_t N, int64_t D, float tau, const float* tau_per_chain, const float* q0,
                    const float* logp0, const float* g0, const float* q1, const float* logp1, const float* g1,
                    float* q_out, float* logp_out, float* g_out, float* acceptance_rate_out,
                    uint8_t* is_accepted_out) {
  BJX_CHECK_ARG(N >= 0 && D > 0, "bjx_mala_finish: bad sizes");
  if (N == 0) return 0;
  BJX_CHECK_ARG(q0 && logp0 && g0 && q1 && logp1 && g1 && q_out && logp_out && g_out && acceptance_rate_out &&
                    is_accepted_out,
                "bjx_mala_finish: null pointer");
#define BJX_MALA_FINISH(KERNEL)                                                                                 \
  BJX_LAUNCH_ROWS(KERNEL, N, stream, Key{key0, key1}, chain_offset, step_fold, N, D, tau, tau_per_chain, q0, logp0, \
                  g0, q1, logp1, g1, q_out, logp_out, g_out, acceptance_rate_out, is_accepted_out)
  if (bjx_vec4_ok(D, q0, g0, q1, g1, q_out, g_out)) {
    if (D <= 256) BJX_MALA_FINISH(k_mala_finish_res<1>);
    else if (D <= 512) BJX_MALA_FINISH(k_mala_finish_res<2>);
    else if (D <= 1024) BJX_MALA_FINISH(k_mala_finish_res<4>);
    else BJX_MALA_FINISH(k_mala_finish<4>);
  } else {
    BJX_MALA_FINISH(k_mala_finish<1>);
  }
#undef BJX_MALA_FINISH
  return bjx_check_launch("bjx_mala_finish");
}

}  // extern "C"
