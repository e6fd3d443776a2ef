// Pretuning arithmetic of SMC (gfx950): what lies between the trial transition of every particle and the new
// per-particle parameter rows.  C ABI in include/bjx_hip.h ("SMC", pretuning).
//
// Reference: blackjax/smc/pretuning.py (esjd, update_parameter_distribution); Fearnhead & Taylor 2013, eq. 4.
//
// Three launches, none of which reads anything back: the expected squared jump distance of every particle (one
// wavefront per row, the row sum in fp64), the weights alpha + measure normalised by one workgroup (the shape of
// bjx_smc_reweight), and the jittered parameter rows gathered by the ancestors drawn from those weights (one wavefront
// per output row, the noise regenerated from the key at the SOURCE row's index: no (N, K) noise array exists).  The
// ancestors themselves are bjx_smc_resample_sorted's.  The order of a workgroup's sums is bjx_smc_dev.h's, the row
// mapping and the normal draws are bjx_rows.h's.
#include <math.h>

#include "../../include/bjx_hip.h"
#include "bjx_device.h"
#include "bjx_host.h"
#include "bjx_rows.h"
#include "bjx_smc_dev.h"

using namespace bjx;

namespace {

constexpr int kRedBlock = 1024;  // the one workgroup of the weights kernel
constexpr int kRedWaves = kRedBlock / BJX_WAVE;
constexpr int64_t kMaxCols = (int64_t)1 << 20;

// pretuning.py::esjd: measure_i = acc_i * sum_j d_j^2 / imm_j with d = prev - next rounded to fp32, the quotients
// and their sum in fp64 (per-lane partials in column order, then wave_sum), the product with acc_i in fp64, rounded
// once.  imm null is the identity metric; otherwise row i reads imm + i * imm_stride.  A measure that is NaN, +-inf
// or negative is stored as exactly 0: the particle then weighs alpha and no sum downstream is poisoned.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_esjd(int64_t N, int64_t D, const float* __restrict__ prev, const float* __restrict__ next,
       const float* __restrict__ acc, const float* __restrict__ imm, int64_t imm_stride,
       float* __restrict__ measure) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = wave_row0(); r < N; r += wave_row_stride()) {
    const float* a = prev + r * D;
    const float* b = next + r * D;
    const float* m = imm ? imm + r * imm_stride : nullptr;
    double s = 0.0;
    for (int64_t j = (int64_t)lane * VEC; j < D; j += 64 * VEC) {
      float av[VEC], bv[VEC], mv[VEC];
      ldv<VEC>(a + j, av);
      ldv<VEC>(b + j, bv);
      if (m) ldv<VEC>(m + j, mv);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const float d = av[e] - bv[e];
        const double d2 = (double)d * (double)d;
        s += m ? d2 / (double)mv[e] : d2;
      }
    }
    s = wave_sum(s);
    const float v = (float)(s * (double)acc[r]);
    if (lane == 0) measure[r] = (v >= 0.0f && v != __builtin_inff()) ? v : 0.0f;  // (a NaN fails v >= 0)
  }
}

// pretuning.py::update_parameter_distribution, the weights: t_i = alpha + measure_i and their sum in fp64,
// w_i = t_i / S rounded once.  S == 0 (alpha 0 and no particle moved) gives uniform weights.
__global__ void __launch_bounds__(kRedBlock)
k_pretune_weights(int64_t N, double alpha, const float* __restrict__ measure, float* __restrict__ w_out) {
  __shared__ double sh[kRedWaves];
  double s = 0.0;
  for (int64_t j = threadIdx.x; j < N; j += kRedBlock) s += alpha + (double)measure[j];
  s = block_sum<kRedWaves>(s, sh);
  const float uniform = (float)(1.0 / (double)N);
  for (int64_t j = threadIdx.x; j < N; j += kRedBlock)
    w_out[j] = s == 0.0 ? uniform : (float)((alpha + (double)measure[j]) / s);
}

// x + sigma * z as one fused multiply-add, or x * exp(sigma * z) with the product and the exponential each rounded to
// fp32 (exp_cr): a parameter that must stay positive keeps its sign whatever z is.
template <bool LOG>
__device__ __forceinline__ float jitter(float p, float sigma, float z) {
  if constexpr (LOG) {
    const float t = sigma * z;
    return p * exp_cr(t);
  } else {
    return fmaf(sigma, z, p);
  }
}

__device__ __forceinline__ int64_t clipped_ancestor(const int32_t* __restrict__ ancestors, int64_t i, int64_t N) {
  const int64_t a = ancestors[i];
  return a < 0 ? 0 : (a > N - 1 ? N - 1 : a);
}

// out[i, k] = jitter(P[a_i, k], sigma_k, normal(key, (N, K))[a_i, k]), one wavefront per output row.  The noise is
// the source row's (the reference adds the noise, then resamples); an ancestor outside [0, N) is clamped as k_gather
// clamps it.
template <int VEC, bool LOG>
__device__ __forceinline__ void jitter_gather_rows(Key key, int64_t N, int64_t M, int64_t K,
                                                   const float* __restrict__ P,
                                                   const int32_t* __restrict__ ancestors,
                                                   const float* __restrict__ sigma, int64_t sigma_stride,
                                                   float* __restrict__ out) {
  const float sigma0 = sigma[0];
  for (int64_t r = wave_row0(); r < M; r += wave_row_stride()) {
    const int64_t a = clipped_ancestor(ancestors, r, N);
    for (int64_t j = (int64_t)(threadIdx.x & 63) * VEC; j < K; j += 64 * VEC) {
      float p[VEC], z[VEC], sg[VEC], o[VEC];
      ldv<VEC>(P + a * K + j, p);
      if (sigma_stride) ldv<VEC>(sigma + j, sg);
      normalv<VEC>(key, a * K + j, z);
#pragma unroll
      for (int e = 0; e < VEC; ++e) o[e] = jitter<LOG>(p[e], sigma_stride ? sg[e] : sigma0, z[e]);
      stv<VEC>(out + r * K + j, o);
    }
  }
}
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_jitter_gather(Key key, int64_t N, int64_t M, int64_t K, const float* __restrict__ P,
                const int32_t* __restrict__ ancestors, const float* __restrict__ sigma, int64_t sigma_stride,
                float* __restrict__ out) {
  jitter_gather_rows<VEC, false>(key, N, M, K, P, ancestors, sigma, sigma_stride, out);
}
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_jitter_gather_log(Key key, int64_t N, int64_t M, int64_t K, const float* __restrict__ P,
                    const int32_t* __restrict__ ancestors, const float* __restrict__ sigma, int64_t sigma_stride,
                    float* __restrict__ out) {
  jitter_gather_rows<VEC, true>(key, N, M, K, P, ancestors, sigma, sigma_stride, out);
}

// K == 1 (a step size per particle): one thread per output row, so that a wavefront draws 64 scalars instead of 1
template <bool LOG>
__global__ void __launch_bounds__(kBlock)
k_jitter_gather_scalar(Key key, int64_t N, int64_t M, const float* __restrict__ P,
                       const int32_t* __restrict__ ancestors, const float* __restrict__ sigma,
                       float* __restrict__ out) {
  const float sigma0 = sigma[0];
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < M; i += (int64_t)gridDim.x * kBlock) {
    const int64_t a = clipped_ancestor(ancestors, i, N);
    out[i] = jitter<LOG>(P[a], sigma0, normal_from_bits(key_bits32(key, (uint64_t)a)));
  }
}

}  // namespace

extern "C" {

int bjx_smc_esjd(void* stream, int64_t N, int64_t D, const float* prev, const float* next, const float* acc,
                 const float* imm, int64_t imm_stride, float* measure_out) {
  BJX_CHECK_ARG(N >= 1 && N <= kMaxParticles && D >= 1 && D <= kMaxCols && (imm_stride == 0 || imm_stride == D),
                "bjx_smc_esjd: bad sizes");
  BJX_CHECK_ARG(prev && next && acc && measure_out, "bjx_smc_esjd: null pointer");
  BJX_LAUNCH_ROWS_VEC(bjx_vec4_ok(D, prev, next, imm), k_esjd, N, stream, N, D, prev, next, acc, imm, imm_stride,
                      measure_out);
  return bjx_check_launch("bjx_smc_esjd");
}

int bjx_smc_pretune_weights(void* stream, int64_t N, float alpha, const float* measure, float* weights_out) {
  BJX_CHECK_ARG(N >= 1 && N <= kMaxParticles && alpha >= 0.0f && alpha <= 3.402823466e38f,
                "bjx_smc_pretune_weights: bad sizes");
  BJX_CHECK_ARG(measure && weights_out, "bjx_smc_pretune_weights: null pointer");
  hipLaunchKernelGGL(k_pretune_weights, dim3(1), dim3(kRedBlock), 0, (hipStream_t)stream, N, (double)alpha, measure,
                     weights_out);
  return bjx_check_launch("bjx_smc_pretune_weights");
}

int bjx_smc_jitter_gather(void* stream, uint32_t key0, uint32_t key1, int64_t N, int64_t M, int64_t K, const float* P,
                          const int32_t* ancestors, const float* sigma, int64_t sigma_stride, int32_t log_space,
                          float* out) {
  BJX_CHECK_ARG(N >= 1 && N <= kMaxParticles && M >= 1 && M <= kMaxParticles && K >= 1 && K <= kMaxCols &&
                    (sigma_stride == 0 || sigma_stride == 1) && (log_space == 0 || log_space == 1),
                "bjx_smc_jitter_gather: bad sizes");
  BJX_CHECK_ARG(P && ancestors && sigma && out, "bjx_smc_jitter_gather: null pointer");
  BJX_CHECK_ARG(P != out, "bjx_smc_jitter_gather: out of place only");
  const Key key{key0, key1};
  if (K == 1) {
    const dim3 grid(bjx_flat_grid(M, kBlock)), block(kBlock);
    if (log_space)
      hipLaunchKernelGGL(k_jitter_gather_scalar<true>, grid, block, 0, (hipStream_t)stream, key, N, M, P, ancestors,
                         sigma, out);
    else
      hipLaunchKernelGGL(k_jitter_gather_scalar<false>, grid, block, 0, (hipStream_t)stream, key, N, M, P, ancestors,
                         sigma, out);
    return bjx_check_launch("bjx_smc_jitter_gather");
  }
  const bool vec4 = bjx_vec4_ok(K, P, out, sigma_stride ? sigma : nullptr);
  if (log_space)
    BJX_LAUNCH_ROWS_VEC(vec4, k_jitter_gather_log, M, stream, key, N, M, K, P, ancestors, sigma, sigma_stride, out);
  else
    BJX_LAUNCH_ROWS_VEC(vec4, k_jitter_gather, M, stream, key, N, M, K, P, ancestors, sigma, sigma_stride, out);
  return bjx_check_launch("bjx_smc_jitter_gather");
}

}  // extern "C"
