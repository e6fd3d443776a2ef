// Marginal latent-Gaussian sampler (gfx950).  C ABI in include/bjx_hip.h ("marginal latent Gaussian").
//
// Reference: blackjax/mcmc/marginal_latent_gaussian.py (init, build_kernel, generate_mean_shifted_logprob), the
// auxiliary marginal sampler of Titsias & Papaspiliopoulos (2018); mcmc/proposal.py::static_binomial_sampling,
// safe_energy_diff.  The prior is N(0, C) with C = U diag(Gamma) U^T; the kernels here work on rows in the prior's
// eigenbasis (U_x = U^T x, U_grad_x = U^T g) and the rotations are bjx_dense.hip's GEMMs.
//
// Layout and mapping: bjx_rows.h.  Bytes per element of each launch (Gamma and shift are (D,), shared by all rows and
// served from cache):
//   bjx_mgrad_propose  r U_x, U_grad_x                    w t                               12   (one normal per element)
//   bjx_mgrad_shift    r y, g                             w g'                              12
//   bjx_mgrad_finish   diagonal prior, resident           r 4 eigenbasis rows, w 2          24
//                      diagonal prior, two-pass           + the two selected rows again     32
//                      dense prior, resident              + r position, gradient, w both    40
//                      dense prior, two-pass                                                48
// The finish kernels are bjx_finish.h's, with the policy MgradFinish below.  VGPRs (kernel-resource-usage remark of
// the gfx950 build), no scratch anywhere: see the kernels, and bjx_finish.h for the finish.
#include <math.h>

#include "../../include/bjx_hip.h"
#include "bjx_device.h"
#include "bjx_finish.h"
#include "bjx_host.h"
#include "bjx_rows.h"

using namespace bjx;

namespace {

// Gamma_1 = Gamma delta / (delta + 2 Gamma), Gamma_3 = (delta + 2 Gamma) / (delta + 4 Gamma), left to right with
// correctly rounded divisions; 2 Gamma and 4 Gamma are exact, so the fmaf is the plain sum.  Computed per element from
// Gamma[j] and the row's delta: a scalar and a per-chain step size share this arithmetic.
__device__ __forceinline__ void mgrad_coef(float gam, float delta, float* g1, float* g3) {
  const float d2 = fmaf(2.0f, gam, delta);
  const float d4 = fmaf(4.0f, gam, delta);
  *g1 = (gam * delta) / d2;
  *g3 = d2 / d4;
}

// t = Gamma_1 (U_x / (0.5 delta) + U_grad_x) + sqrt(Gamma_2) normal(y_key, (D,)), Gamma_2 = Gamma_1 / Gamma_3;
// y_key = split(chain key, 2)[0].  The position of the proposal is y = U t (the caller's GEMM; y = t for a diagonal
// prior).  Reads U_x, U_grad_x, writes t: bjx_mala_propose's traffic and its one normal per element, the operands
// requested before the RNG arithmetic.  VEC = 4 / 1: 76 / 56 VGPRs.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_mgrad_propose(Key key, int64_t off, int64_t fold, int64_t N, int64_t D, float delta_s,
                const float* __restrict__ delta_pc, const float* __restrict__ gamma, const float* __restrict__ ux,
                const float* __restrict__ ugx, float* __restrict__ t_out) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = wave_row0(); r < N; r += wave_row_stride()) {
    const Key kc = chain_key(key, (uint64_t)(r + off), fold);
    const Key kn = key_child(kc, 0);  // y_key, u_key = split(rng_key)
    const float delta = delta_pc ? delta_pc[r] : delta_s;
    const float hd = 0.5f * delta;
    const int64_t base = r * D;
    for (int64_t j = (int64_t)lane * VEC; j < D; j += 64 * VEC) {
      float a[VEC], b[VEC], gam[VEC], z[VEC], t[VEC];
      ldv<VEC>(ux + base + j, a);
      ldv<VEC>(ugx + base + j, b);
      ldv<VEC>(gamma + j, gam);
      normalv<VEC>(kn, j, z);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        float g1, g3;
        mgrad_coef(gam[e], delta, &g1, &g3);
        const float s = sqrtf(g1 / g3);
        t[e] = fmaf(s, z[e], g1 * (a[e] / hd + b[e]));
      }
      stv<VEC>(t_out + base + j, t);
    }
  }
}

// generate_mean_shifted_logprob: logp' = logp + dot(y, shift) (fp64 sum rounded once), g' = g + shift, out of place.
// VEC = 4 / 1: 52 / 30 VGPRs.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_mgrad_shift(int64_t N, int64_t D, const float* __restrict__ shift, const float* __restrict__ y,
              const float* __restrict__ logp, const float* __restrict__ g, float* __restrict__ logp_out,
              float* __restrict__ g_out) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = wave_row0(); r < N; r += wave_row_stride()) {
    const int64_t base = r * D;
    double acc = 0.0;
    for (int64_t j = (int64_t)lane * VEC; j < D; j += 64 * VEC) {
      float yy[VEC], gg[VEC], sh[VEC], go[VEC];
      ldv<VEC>(y + base + j, yy);
      ldv<VEC>(g + base + j, gg);
      ldv<VEC>(shift + j, sh);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        acc += (double)yy[e] * (double)sh[e];
        go[e] = gg[e] + sh[e];
      }
      stv<VEC>(g_out + base + j, go);
    }
    acc = wave_sum(acc);
    if (lane == 0) logp_out[r] = logp[r] + (float)acc;
  }
}

// The finish policy (bjx_finish.h).  The row pair is the eigenbasis pair (a = U_x / U_y, b = U_grad_x / U_grad_y), aux is
// Gamma and the sums are the two dots of the acceptance ratio:
//   t_x = Gamma_1 (U_x / (0.5 delta) + 0.5 U_grad_x), t_y likewise from the proposal
//   hxy += (U_x - t_y) (Gamma_3 U_grad_y) ; hyx += (U_y - t_x) (Gamma_3 U_grad_x)      (fp32 factors, fp64 products)
//   log_ratio = ((logp_y - logp_x) + hxy) - hyx
// With a dense prior (x_out non-null) the state has position and gradient beside their eigenbasis images, the carried
// pair; with a diagonal prior they are the same arrays and only the eigenbasis pair is written.
struct MgradFinish {
  float delta_s;
  const float* delta_pc;
  struct Row {
    float delta, hd;
  };
  static constexpr int kSums = 2;
  static constexpr bool kAux = true;
  __device__ __forceinline__ Row row(int64_t r) const {
    const float delta = delta_pc ? delta_pc[r] : delta_s;
    return {delta, 0.5f * delta};
  }
  static __device__ __forceinline__ void term(Row row, float gam, float ux, float uy, float ugx, float ugy, double& hxy,
                                              double& hyx) {
    float g1, g3;
    mgrad_coef(gam, row.delta, &g1, &g3);
    const float tx = g1 * fmaf(0.5f, ugx, ux / row.hd);
    const float ty = g1 * fmaf(0.5f, ugy, uy / row.hd);
    hxy += (double)(ux - ty) * (double)(g3 * ugy);
    hyx += (double)(uy - tx) * (double)(g3 * ugx);
  }
  static __device__ __forceinline__ float delta(Row, double hxy, double hyx, float lpx, float lpy) {
    const float lr = ((lpy - lpx) + (float)hxy) - (float)hyx;
    return safe_energy_diff(lr);
  }
};
template <int VEC> constexpr auto k_mgrad_finish = k_finish<VEC, MgradFinish>;
template <int NI> constexpr auto k_mgrad_finish_res = k_finish_res<NI, MgradFinish>;

}  // namespace

extern "C" {

int bjx_mgrad_propose(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold,
                      int64_t N, int64_t D, float delta, const float* delta_per_chain, const float* gamma,
                      const float* u_x, const float* u_grad_x, float* t_out) {
  BJX_CHECK_ARG(N >= 0 && D > 0, "bjx_mgrad_propose: bad sizes");
  if (N == 0) return 0;
  BJX_CHECK_ARG(gamma && u_x && u_grad_x && t_out, "bjx_mgrad_propose: null pointer");
  BJX_LAUNCH_ROWS_VEC(bjx_vec4_ok(D, gamma, u_x, u_grad_x, t_out), k_mgrad_propose, N, stream, Key{key0, key1},
                      chain_offset, step_fold, N, D, delta, delta_per_chain, gamma, u_x, u_grad_x, t_out);
  return bjx_check_launch("bjx_mgrad_propose");
}

int bjx_mgrad_shift(void* stream, int64_t N, int64_t D, const float* shift, const float* y, const float* logp,
                    const float* g, float* logp_out, float* g_out) {
  BJX_CHECK_ARG(N >= 0 && D > 0, "bjx_mgrad_shift: bad sizes");
  if (N == 0) return 0;
  BJX_CHECK_ARG(shift && y && logp && g && logp_out && g_out, "bjx_mgrad_shift: null pointer");
  BJX_CHECK_ARG(g_out != g && g_out != y && logp_out != logp, "bjx_mgrad_shift: outputs must not alias inputs");
  BJX_LAUNCH_ROWS_VEC(bjx_vec4_ok(D, shift, y, g, g_out), k_mgrad_shift, N, stream, N, D, shift, y, logp, g, logp_out,
                      g_out);
  return bjx_check_launch("bjx_mgrad_shift");
}

int bjx_mgrad_finish(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold, int64_t N,
                     int64_t D, float delta, const float* delta_per_chain, const float* gamma, const float* x,
                     const float* logp_x, const float* g_x, const float* u_x, const float* u_grad_x, const float* y,
                     const float* logp_y, const float* g_y, const float* u_y, const float* u_grad_y, float* x_out,
                     float* logp_out, float* g_out, float* u_x_out, float* u_grad_x_out, float* acceptance_rate_out,
                     uint8_t* is_accepted_out) {
  BJX_CHECK_ARG(N >= 0 && D > 0, "bjx_mgrad_finish: bad sizes");
  if (N == 0) return 0;
  BJX_CHECK_ARG(gamma && logp_x && u_x && u_grad_x && logp_y && u_y && u_grad_y && logp_out && u_x_out &&
                    u_grad_x_out && acceptance_rate_out && is_accepted_out,
                "bjx_mgrad_finish: null pointer");
  const bool dense = x_out != nullptr;
  BJX_CHECK_ARG(dense ? (x && g_x && y && g_y && g_out) : (!x && !g_x && !y && !g_y && !g_out),
                "bjx_mgrad_finish: x, g_x, y, g_y, x_out, g_out are given together (dense prior) or not at all");
  BJX_LAUNCH_ROWS_RES(
      bjx_vec4_ok(D, gamma, x, g_x, u_x, u_grad_x, y, g_y, u_y, u_grad_y, x_out, g_out, u_x_out, u_grad_x_out), D,
      k_mgrad_finish_res, k_mgrad_finish, N, stream, Key{key0, key1}, chain_offset, step_fold, N, D,
      MgradFinish{delta, delta_per_chain}, u_x, logp_x, u_grad_x, u_y, logp_y, u_grad_y, u_x_out, logp_out, u_grad_x_out,
      acceptance_rate_out, is_accepted_out, gamma, x, g_x, y, g_y, x_out, g_out);
  return bjx_check_launch("bjx_mgrad_finish");
}

}  // extern "C"
