// Barker proposal sampler (gfx950).  C ABI in include/bjx_hip.h ("Barker").
//
// Reference: blackjax/mcmc/barker.py (init, build_kernel: _barker_sample_nd, _barker_logpdf, kernel) with a
// diagonal preconditioner, mcmc/proposal.py::compute_asymmetric_acceptance_ratio, static_binomial_sampling,
// safe_energy_diff.  Livingstone & Zanella 2022.
//
// Layout and mapping: bjx_rows.h.  A transition is propose -> user callable -> finish:
// 12 (16 with a per-chain metric) + 8 + 24 bytes per element.  The finish kernels are bjx_finish.h's, with the policy
// BarkerFinish below.
#include <math.h>

#include "../../include/bjx_hip.h"
#include "bjx_device.h"
#include "bjx_finish.h"
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

// The finish policy (bjx_finish.h): no per-row scalar, one sum, the accept on safe_energy_diff of the log ratio.
struct BarkerFinish {
  struct Row {};
  static constexpr int kSums = 1;
  static constexpr bool kAux = false;
  __device__ __forceinline__ Row row(int64_t) const { return {}; }
  static __device__ __forceinline__ void term(Row, float, float a0, float a1, float b0, float b1, double& sum,
                                              double&) {
    sum += barker_term(a0, a1, b0, b1);
  }
  static __device__ __forceinline__ float delta(Row, double sum, double, float lp0, float lp1) {
    const float log_ratio = (lp1 - lp0) + (float)sum;
    return safe_energy_diff(log_ratio);
  }
};
template <int VEC> constexpr auto k_barker_finish = k_finish<VEC, BarkerFinish>;
template <int NI> constexpr auto k_barker_finish_res = k_finish_res<NI, BarkerFinish>;

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
  // no shared operand and no carried pair: the seven nullptr
  BJX_LAUNCH_ROWS_RES(bjx_vec4_ok(D, q0, g0, q1, g1, q_out, g_out), D, k_barker_finish_res, k_barker_finish, N, stream,
                      Key{key0, key1}, chain_offset, step_fold, N, D, BarkerFinish{}, q0, logp0, g0, q1, logp1, g1, q_out,
                      logp_out, g_out, acceptance_rate_out, is_accepted_out, nullptr, nullptr, nullptr, nullptr, nullptr,
                      nullptr, nullptr);
  return bjx_check_launch("bjx_barker_finish");
}

}  // extern "C"
