// Random-walk Metropolis family: rmh, additive_step_random_walk, irmh (gfx950).  C ABI in include/bjx_hip.h
// ("random walk").
//
// Reference: blackjax/mcmc/random_walk.py (init, normal, build_additive_step, build_rmh: transition_energy, kernel,
// rmh_proposal), blackjax/mcmc/irmh.py (build_kernel), blackjax/util.py::generate_gaussian_noise,
// mcmc/proposal.py::compute_asymmetric_acceptance_ratio, static_binomial_sampling, safe_energy_diff.
//
// Layout and mapping: bjx_rows.h.  A transition is propose -> user callable (value only) -> finish:
// 8 + 4 + 8 = 20 bytes per element, no gradient anywhere.
#include <math.h>

#include "../../include/bjx_hip.h"
#include "bjx_device.h"
#include "bjx_host.h"
#include "bjx_rows.h"

using namespace bjx;

namespace {

// The two keys of a transition: key_proposal, key_accept = split(chain key, 2) (random_walk.py, irmh.py kernel);
// metropolis_accept draws from the second.
enum { kKeyProposal = 0 };

// out[r] = normal(k_r, (D,)) with k_r the chain key (child < 0) or its child: a user generator's draw
// (random.chain_normal) and the left operand of the dense step's product.  4 B written per element.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_rw_noise(Key key, int64_t off, int64_t fold, int child, int64_t N, int64_t D, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = wave_row0(); r < N; r += wave_row_stride()) {
    Key kn = chain_key(key, (uint64_t)(r + off), fold);
    if (child >= 0) kn = key_child(kn, (uint64_t)child);
    const int64_t base = r * D;
    for (int64_t j = (int64_t)lane * VEC; j < D; j += 64 * VEC) {
      float z[VEC];
      normalv<VEC>(kn, j, z);
      stv<VEC>(out + base + j, z);
    }
  }
}

// random_walk.py::normal + build_additive_step: q1 = q0 + sigma * normal(key_proposal, (D,)), one fmaf per element;
// sigma is one scalar or one scale per dimension.  Reads q0, writes q1 (8 B per element, plus the (D,) scales from
// cache); bound by the RNG arithmetic of one normal per element (threefry + erf_inv), as k_mala_propose is -- the
// operand is requested before it.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_rw_propose(Key key, int64_t off, int64_t fold, int64_t N, int64_t D, float sigma_s,
             const float* __restrict__ sigma_diag, const float* __restrict__ q0, float* __restrict__ q1_out) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = wave_row0(); r < N; r += wave_row_stride()) {
    const Key kn = key_child(chain_key(key, (uint64_t)(r + off), fold), kKeyProposal);
    const int64_t base = r * D;
    for (int64_t j = (int64_t)lane * VEC; j < D; j += 64 * VEC) {
      float qq[VEC], s[VEC], z[VEC], qn[VEC];
      ldv<VEC>(q0 + base + j, qq);
      if (sigma_diag) {
        ldv<VEC>(sigma_diag + j, s);
      } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) s[e] = sigma_s;
      }
      normalv<VEC>(kn, j, z);
#pragma unroll
      for (int e = 0; e < VEC; ++e) qn[e] = fmaf(s[e], z[e], qq[e]);
      stv<VEC>(q1_out + base + j, qn);
    }
  }
}

// The dense step: q1 = q0 + move_lin, move_lin[r] = sigma @ normal(key_proposal, (D,)) ready in memory (k_rw_noise +
// the MFMA GEMM).  8 B read + 4 B written per element.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_rw_propose_lin(int64_t N, int64_t D, const float* __restrict__ move_lin, const float* __restrict__ q0,
                 float* __restrict__ q1_out) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = wave_row0(); r < N; r += wave_row_stride()) {
    const int64_t base = r * D;
    for (int64_t j = (int64_t)lane * VEC; j < D; j += 64 * VEC) {
      float qq[VEC], mv[VEC], qn[VEC];
      ldv<VEC>(q0 + base + j, qq);
      ldv<VEC>(move_lin + base + j, mv);
#pragma unroll
      for (int e = 0; e < VEC; ++e) qn[e] = qq[e] + mv[e];
      stv<VEC>(q1_out + base + j, qn);
    }
  }
}

// random_walk.py::build_rmh (transition_energy, kernel) with metropolis_accept on safe_energy_diff.
// f_ip[r] = proposal_logdensity_fn(initial, proposed),
// f_pi[r] = proposal_logdensity_fn(proposed, initial); both null for a symmetric proposal.  Every lane computes the
// row's scalars, lane 0 writes them; the select then reads ONLY the chosen source row (the branch is wave-uniform)
// and writes it out of place: 4 B read + 4 B written per element.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_rw_finish(Key key, int64_t off, int64_t fold, int64_t N, int64_t D, const float* __restrict__ q0,
            const float* __restrict__ logp0, const float* __restrict__ q1, const float* __restrict__ logp1,
            const float* __restrict__ f_ip, const float* __restrict__ f_pi, float* __restrict__ q_out,
            float* __restrict__ logp_out, float* __restrict__ acc_rate_out, uint8_t* __restrict__ is_acc_out) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = wave_row0(); r < N; r += wave_row_stride()) {
    const float lp0 = logp0[r], lp1 = logp1[r];
    float e_init = -lp0, e_new = -lp1;
    if (f_ip) {
      e_init = e_init - f_ip[r];  // transition_energy(initial, proposed)
      e_new = e_new - f_pi[r];    // transition_energy(proposed, initial)
    }
    float p_acc;
    const bool accept = metropolis_accept(key, r + off, fold, safe_energy_diff(e_init - e_new), &p_acc);
    if (lane == 0) {
      acc_rate_out[r] = p_acc;
      is_acc_out[r] = accept ? 1 : 0;
      logp_out[r] = accept ? lp1 : lp0;
    }
    const int64_t base = r * D;
    const float* qs = accept ? q1 : q0;
    for (int64_t j = (int64_t)lane * VEC; j < D; j += 64 * VEC) {
      float a[VEC];
      ldv<VEC>(qs + base + j, a);
      stv<VEC>(q_out + base + j, a);
    }
  }
}

}  // namespace

extern "C" {

int bjx_rw_noise(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold, int32_t child,
                 int64_t N, int64_t D, float* out) {
  BJX_CHECK_ARG(N >= 0 && D > 0 && child >= -1 && child <= 1, "bjx_rw_noise: bad sizes");
  if (N == 0) return 0;
  BJX_CHECK_ARG(out, "bjx_rw_noise: null pointer");
  BJX_LAUNCH_ROWS_VEC(bjx_vec4_ok(D, out), k_rw_noise, N, stream, Key{key0, key1}, chain_offset, step_fold,
                      (int)child, N, D, out);
  return bjx_check_launch("bjx_rw_noise");
}

int bjx_rw_propose(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold, int64_t N,
                   int64_t D, float sigma, const float* sigma_diag, const float* move_lin, const float* q0,
                   float* q1_out) {
  BJX_CHECK_ARG(N >= 0 && D > 0, "bjx_rw_propose: bad sizes");
  if (N == 0) return 0;
  BJX_CHECK_ARG(q0 && q1_out, "bjx_rw_propose: null pointer");
  BJX_CHECK_ARG(!(sigma_diag && move_lin), "bjx_rw_propose: sigma_diag and move_lin are exclusive");
  BJX_CHECK_ARG(q0 != q1_out, "bjx_rw_propose: out of place only");
  const bool v4 = bjx_vec4_ok(D, sigma_diag, move_lin, q0, q1_out);
  if (move_lin)
    BJX_LAUNCH_ROWS_VEC(v4, k_rw_propose_lin, N, stream, N, D, move_lin, q0, q1_out);
  else
    BJX_LAUNCH_ROWS_VEC(v4, k_rw_propose, N, stream, Key{key0, key1}, chain_offset, step_fold, N, D, sigma,
                        sigma_diag, q0, q1_out);
  return bjx_check_launch("bjx_rw_propose");
}

int bjx_rw_finish(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold, int64_t N,
                  int64_t D, const float* q0, const float* logp0, const float* q1, const float* logp1,
                  const float* f_init_prop, const float* f_prop_init, float* q_out, float* logp_out,
                  float* acceptance_rate_out, uint8_t* is_accepted_out) {
  BJX_CHECK_ARG(N >= 0 && D > 0, "bjx_rw_finish: bad sizes");
  if (N == 0) return 0;
  BJX_CHECK_ARG(q0 && logp0 && q1 && logp1 && q_out && logp_out && acceptance_rate_out && is_accepted_out,
                "bjx_rw_finish: null pointer");
  BJX_CHECK_ARG((f_init_prop == nullptr) == (f_prop_init == nullptr),
                "bjx_rw_finish: f_init_prop and f_prop_init go together");
  BJX_CHECK_ARG(q_out != q0 && q_out != q1 && logp_out != logp0 && logp_out != logp1,
                "bjx_rw_finish: out of place only");
  BJX_LAUNCH_ROWS_VEC(bjx_vec4_ok(D, q0, q1, q_out), k_rw_finish, N, stream, Key{key0, key1}, chain_offset,
                      step_fold, N, D, q0, logp0, q1, logp1, f_init_prop, f_prop_init, q_out, logp_out,
                      acceptance_rate_out, is_accepted_out);
  return bjx_check_launch("bjx_rw_finish");
}

}  // extern "C"
