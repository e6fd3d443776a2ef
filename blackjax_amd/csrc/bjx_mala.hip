// Metropolis-adjusted Langevin algorithm (gfx950).  C ABI in include/bjx_hip.h ("MALA").
//
// Reference: blackjax/mcmc/mala.py (init, build_kernel: transition_energy, kernel),
// mcmc/diffusions.py::overdamped_langevin, mcmc/proposal.py::compute_asymmetric_acceptance_ratio,
// static_binomial_sampling, safe_energy_diff.
//
// Layout and mapping: bjx_rows.h.  A transition is propose -> user callable -> finish: 12 + 8 + 24 = 44 bytes
// per element.  The finish kernels are bjx_finish.h's, with the policy MalaFinish below.
#include <math.h>

#include "../../include/bjx_hip.h"
#include "bjx_device.h"
#include "bjx_finish.h"
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

// The finish policy (bjx_finish.h).  mala.py transition_energy: -logp(new) + 0.25 * (1 / tau) * sum theta^2 with
// theta = state.position - new.position - tau * new.grad; the accept is on
// safe_energy_diff(E(new, state) - E(state, new)) and the two sums are the theta^2 of E(state, new) and E(new, state).
struct MalaFinish {
  float tau_s;
  const float* tau_pc;
  struct Row {
    float tau, ntau;
  };
  static constexpr int kSums = 2;
  static constexpr bool kAux = false;
  __device__ __forceinline__ Row row(int64_t r) const {
    const float tau = tau_pc ? tau_pc[r] : tau_s;
    return {tau, -tau};
  }
  static __device__ __forceinline__ void term(Row row, float, float a0, float a1, float b0, float b1,
                                              double& sum_new, double& sum_prev) {
    const float tn = fmaf(row.ntau, b1, a0 - a1);
    const float tp = fmaf(row.ntau, b0, a1 - a0);
    sum_new += (double)tn * (double)tn;
    sum_prev += (double)tp * (double)tp;
  }
  static __device__ __forceinline__ float delta(Row row, double sum_new, double sum_prev, float lp0, float lp1) {
    const float c = 0.25f * (1.0f / row.tau);  // two fp32 roundings, as written in mala.py
    const float e_new = fmaf(c, (float)sum_new, -lp1);    // transition_energy(state, new_state)
    const float e_prev = fmaf(c, (float)sum_prev, -lp0);  // transition_energy(new_state, state)
    return safe_energy_diff(e_prev - e_new);
  }
};
template <int VEC> constexpr auto k_mala_finish = k_finish<VEC, MalaFinish>;
template <int NI> constexpr auto k_mala_finish_res = k_finish_res<NI, MalaFinish>;

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
  // no shared operand and no carried pair: the seven nullptr
  BJX_LAUNCH_ROWS_RES(bjx_vec4_ok(D, q0, g0, q1, g1, q_out, g_out), D, k_mala_finish_res, k_mala_finish, N, stream,
                      Key{key0, key1}, chain_offset, step_fold, N, D, MalaFinish{tau, tau_per_chain}, q0, logp0, g0, q1,
                      logp1, g1, q_out, logp_out, g_out, acceptance_rate_out, is_accepted_out, nullptr, nullptr, nullptr,
                      nullptr, nullptr, nullptr, nullptr);
  return bjx_check_launch("bjx_mala_finish");
}

}  // extern "C"
