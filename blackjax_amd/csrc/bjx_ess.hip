// Elliptical slice sampler (gfx950).  C ABI in include/bjx_hip.h ("elliptical slice").
//
// Reference: blackjax/mcmc/elliptical_slice.py (init, build_kernel: kernel, elliptical_proposal: slice_fn, ellipsis),
// blackjax/util.py::generate_gaussian_noise.
//
// Layout and mapping: bjx_rows.h.  A transition is
//   begin -> user callable -> { shrink -> user callable } until no chain is live.
// Bytes per element: begin (diagonal prior) 4 read + 8 written and one normal draw -- bjx_mala_propose's profile;
// begin (dense prior) 8 + 8; shrink of a live row 8 read + 4 written; shrink of a row that accepts 8 read + 4
// written, once; a finished row one byte per launch.
#include <math.h>

#include "../../include/bjx_hip.h"
#include "bjx_device.h"
#include "bjx_host.h"
#include "bjx_rows.h"

using namespace bjx;

namespace {

// The four keys of a transition: key_slice, key_momentum, key_uniform, key_theta = split(chain key, 4).
enum { kKeySlice = 0, kKeyMomentum = 1, kKeyUniform = 2, kKeyTheta = 3 };

constexpr float kTwoPi = 6.28318530717958647692f;  // f32(2 pi)

// cos, sin of (double)theta, each rounded once to fp32
__device__ __forceinline__ void ellipse_cs(float theta, float* c, float* s) {
  double sd, cd;
  sincos((double)theta, &sd, &cd);
  *c = (float)cd;
  *s = (float)sd;
}

// elliptical_slice.py::ellipsis, position: fma(nu - mean, s, (q0 - mean) * c) + mean
__device__ __forceinline__ float ellipse_p(float q, float nu, float mu, float c, float s) {
  const float a = q - mu, b = nu - mu;
  return fmaf(b, s, a * c) + mu;
}
// elliptical_slice.py::ellipsis, momentum: fma(-(q0 - mean), s, (nu - mean) * c) + mean
__device__ __forceinline__ float ellipse_m(float q, float nu, float mu, float c, float s) {
  const float a = q - mu, b = nu - mu;
  return fmaf(-a, s, b * c) + mu;
}

// Opening of a transition.  DENSE: nu = nu_lin + mean with nu_lin = normal(key_momentum) @ L^T ready in memory;
// otherwise nu = fma(sqrt(cov_j), normal(key_momentum, (D,))_j, mean_j) drawn here.  Writes nu, the slice height
// logy = logp0 + log(uniform(key_uniform)), the first angle theta = 2 pi uniform(key_theta) with its bracket
// [theta - 2 pi, theta], subiter = 1, done = 0 and the first proposal.
template <int VEC, bool DENSE>
__global__ void __launch_bounds__(kBlock)
k_ess_begin(Key key, int64_t off, int64_t fold, int64_t N, int64_t D, const float* __restrict__ mean,
            const float* __restrict__ cov_diag, const float* __restrict__ nu_lin, const float* __restrict__ q0,
            const float* __restrict__ logp0, float* __restrict__ nu_out, float* __restrict__ q_prop,
            float* __restrict__ logy, float* __restrict__ theta, float* __restrict__ theta_min,
            float* __restrict__ theta_max, int32_t* __restrict__ subiter, uint8_t* __restrict__ done) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = wave_row0(); r < N; r += wave_row_stride()) {
    const Key kc = chain_key(key, (uint64_t)(r + off), fold);
    const Key kn = key_child(kc, kKeyMomentum);
    const float th = kTwoPi * key_uniform(key_child(kc, kKeyTheta));
    float c, s;
    ellipse_cs(th, &c, &s);
    if (lane == 0) {
      const float u = key_uniform(key_child(kc, kKeyUniform));
      logy[r] = logp0[r] + (float)log((double)u);  // u = 0: -inf
      theta[r] = th;
      theta_min[r] = th - kTwoPi;
      theta_max[r] = th;
      subiter[r] = 1;
      done[r] = 0;
    }
    const int64_t base = r * D;
    for (int64_t j = (int64_t)lane * VEC; j < D; j += 64 * VEC) {
      float qq[VEC], mu[VEC], nu[VEC], pp[VEC];
      ldv<VEC>(q0 + base + j, qq);
      ldv<VEC>(mean + j, mu);
      if constexpr (DENSE) {
        float nl[VEC];
        ldv<VEC>(nu_lin + base + j, nl);
#pragma unroll
        for (int e = 0; e < VEC; ++e) nu[e] = nl[e] + mu[e];
      } else {
        float cv[VEC], z[VEC];
        ldv<VEC>(cov_diag + j, cv);
        normalv<VEC>(kn, j, z);
#pragma unroll
        for (int e = 0; e < VEC; ++e) nu[e] = fmaf(sqrtf(cv[e]), z[e], mu[e]);
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) pp[e] = ellipse_p(qq[e], nu[e], mu[e], c, s);
      stv<VEC>(nu_out + base + j, nu);
      stv<VEC>(q_prop + base + j, pp);
    }
  }
}

// n[r] = normal(key_momentum of chain r, (D,)): the A operand of the dense prior's GEMM.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_ess_noise(Key key, int64_t off, int64_t fold, int64_t N, int64_t D, float* __restrict__ n_out) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = wave_row0(); r < N; r += wave_row_stride()) {
    const Key kn = key_child(chain_key(key, (uint64_t)(r + off), fold), kKeyMomentum);
    const int64_t base = r * D;
    for (int64_t j = (int64_t)lane * VEC; j < D; j += 64 * VEC) {
      float z[VEC];
      normalv<VEC>(kn, j, z);
      stv<VEC>(n_out + base + j, z);
    }
  }
}

// One round of the slice loop, given the log-likelihood of every row's current proposal.  A finished row costs one
// byte.  A row whose proposal is on the slice -- the reference's loop condition `logp <= logy` is false, which a NaN
// logp makes it too -- latches its outputs, writes its momentum and is finished: its q_prop row is its new position.
// Any other row draws theta = uniform(fold_in(key_slice, subiter), theta_min, theta_max), overwrites its proposal,
// shrinks the bracket towards 0 and counts itself in n_live (one atomic per wave).  Every lane reads the row's scalars
// before lane 0 overwrites them: one wave, one instruction stream, loads ahead of the stores in program order.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_ess_shrink(Key key, int64_t off, int64_t fold, int64_t N, int64_t D, const float* __restrict__ mean,
             const float* __restrict__ q0, const float* __restrict__ nu, const float* __restrict__ logp_prop,
             const float* __restrict__ logy, float* __restrict__ theta, float* __restrict__ theta_min,
             float* __restrict__ theta_max, int32_t* __restrict__ subiter, uint8_t* __restrict__ done,
             float* __restrict__ q_prop, float* __restrict__ logdensity_out, float* __restrict__ theta_out,
             int32_t* __restrict__ subiter_out, float* __restrict__ momentum_out, int32_t* __restrict__ n_live) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = wave_row0(); r < N; r += wave_row_stride()) {
    if (done[r]) continue;
    const float lp = logp_prop[r];
    const int32_t it = subiter[r];
    const bool live = lp <= logy[r];
    float th = theta[r];
    if (live) {
      const Key ks = key_child(chain_key(key, (uint64_t)(r + off), fold), kKeySlice);
      const float lo = theta_min[r], hi = theta_max[r];
      // jax.random.uniform(fold_in(key_slice, subiter), minval=lo, maxval=hi)
      th = fmaxf(lo, fmaf(unit_float(key_bits32(key_child(ks, (uint64_t)(uint32_t)it), 0)), hi - lo, lo));
      if (lane == 0) {
        theta[r] = th;
        if (th < 0.0f) theta_min[r] = th;
        if (th > 0.0f) theta_max[r] = th;
        subiter[r] = it + 1;
        atomicAdd(n_live, 1);
      }
    } else if (lane == 0) {
      logdensity_out[r] = lp;
      theta_out[r] = th;
      subiter_out[r] = it;
      done[r] = 1;
    }
    float c, s;
    ellipse_cs(th, &c, &s);
    float* dst = live ? q_prop : momentum_out;
    const int64_t base = r * D;
    for (int64_t j = (int64_t)lane * VEC; j < D; j += 64 * VEC) {
      float qq[VEC], nn[VEC], mu[VEC], o[VEC];
      ldv<VEC>(q0 + base + j, qq);
      ldv<VEC>(nu + base + j, nn);
      ldv<VEC>(mean + j, mu);
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        o[e] = live ? ellipse_p(qq[e], nn[e], mu[e], c, s) : ellipse_m(qq[e], nn[e], mu[e], c, s);
      stv<VEC>(dst + base + j, o);
    }
  }
}

}  // namespace

extern "C" {

int bjx_ess_begin(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold, int64_t N,
                  int64_t D, const float* mean, const float* cov_diag, const float* nu_lin, const float* q0,
                  const float* logp0, float* nu_out, float* q_prop_out, float* logy_out, float* theta_out,
                  float* theta_min_out, float* theta_max_out, int32_t* subiter_out, uint8_t* done_out) {
  BJX_CHECK_ARG(N >= 0 && D > 0, "bjx_ess_begin: bad sizes");
  if (N == 0) return 0;
  BJX_CHECK_ARG(mean && q0 && logp0 && nu_out && q_prop_out && logy_out && theta_out && theta_min_out &&
                    theta_max_out && subiter_out && done_out,
                "bjx_ess_begin: null pointer");
  BJX_CHECK_ARG((cov_diag != nullptr) != (nu_lin != nullptr),
                "bjx_ess_begin: exactly one of cov_diag and nu_lin must be given");
#define BJX_ESS_BEGIN(VEC, DENSE)                                                                                 \
  BJX_LAUNCH_ROWS((k_ess_begin<VEC, DENSE>), N, stream, Key{key0, key1}, chain_offset, step_fold, N, D, mean,     \
                  cov_diag, nu_lin, q0, logp0, nu_out, q_prop_out, logy_out, theta_out, theta_min_out, theta_max_out, \
                  subiter_out, done_out)
  const bool v4 = bjx_vec4_ok(D, mean, cov_diag, nu_lin, q0, nu_out, q_prop_out);
  if (nu_lin) {
    if (v4) BJX_ESS_BEGIN(4, true);
    else BJX_ESS_BEGIN(1, true);
  } else {
    if (v4) BJX_ESS_BEGIN(4, false);
    else BJX_ESS_BEGIN(1, false);
  }
#undef BJX_ESS_BEGIN
  return bjx_check_launch("bjx_ess_begin");
}

int bjx_ess_noise(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold, int64_t N,
                  int64_t D, float* n_out) {
  BJX_CHECK_ARG(N >= 0 && D > 0, "bjx_ess_noise: bad sizes");
  if (N == 0) return 0;
  BJX_CHECK_ARG(n_out, "bjx_ess_noise: null pointer");
  BJX_LAUNCH_ROWS_VEC(bjx_vec4_ok(D, n_out), k_ess_noise, N, stream, Key{key0, key1}, chain_offset, step_fold, N, D,
                      n_out);
  return bjx_check_launch("bjx_ess_noise");
}

int bjx_ess_shrink(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold, int64_t N,
                   int64_t D, const float* mean, const float* q0, const float* nu, const float* logp_prop,
                   const float* logy, float* theta, float* theta_min, float* theta_max, int32_t* subiter,
                   uint8_t* done, float* q_prop, float* logdensity_out, float* theta_out, int32_t* subiter_out,
                   float* momentum_out, int32_t* n_live) {
  BJX_CHECK_ARG(N >= 0 && D > 0, "bjx_ess_shrink: bad sizes");
  if (N == 0) return 0;
  BJX_CHECK_ARG(mean && q0 && nu && logp_prop && logy && theta && theta_min && theta_max && subiter && done &&
                    q_prop && logdensity_out && theta_out && subiter_out && momentum_out && n_live,
                "bjx_ess_shrink: null pointer");
  BJX_LAUNCH_ROWS_VEC(bjx_vec4_ok(D, mean, q0, nu, q_prop, momentum_out), k_ess_shrink, N, stream, Key{key0, key1},
                      chain_offset, step_fold, N, D, mean, q0, nu, logp_prop, logy, theta, theta_min, theta_max,
                      subiter, done, q_prop, logdensity_out, theta_out, subiter_out, momentum_out, n_live);
  return bjx_check_launch("bjx_ess_shrink");
}

}  // extern "C"
