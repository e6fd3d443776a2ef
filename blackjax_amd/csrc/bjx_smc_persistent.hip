// Persistent-sampling SMC arithmetic (gfx950).  C ABI in include/bjx_hip.h ("SMC", persistent sampling).
//
// Reference: blackjax/smc/persistent_sampling.py (compute_log_persistent_weights, compute_log_Z, step),
// smc/adaptive_persistent_sampling.py (calculate_lambda, build_kernel), smc/ess.py (log_ess), smc/solver.py (dichotomy).
//
// Every iteration weighs the P = i * N particles of all earlier iterations, so unlike the one-workgroup reductions of
// bjx_smc.hip these use the whole device.  A reduction is launch-separated, as the prefix scan is: one workgroup per
// tile of kSmcTile particles writes the tile's (max, S1, S2) in fp64, S_k = sum exp(k (lw - max)) against the tile's
// OWN maximum, and a later launch of one workgroup rescales and adds the tile triples.  The tiling is fixed by P alone
// (never by the grid) and every sum has a fixed tree, so results are reproducible bit for bit; no workgroup waits on
// another.  An evaluation of the bisection's f is one such pair of launches; the bracket lives in the workspace, so
// the number of launches does not depend on the data and nothing is read back by the host.  Which log-weights count,
// the order of a workgroup's sums and the tile size are bjx_smc_dev.h's, shared with bjx_smc.hip.
#include <math.h>

#include "../../include/bjx_hip.h"
#include "bjx_device.h"
#include "bjx_host.h"
#include "bjx_rows.h"
#include "bjx_smc_dev.h"

using namespace bjx;

namespace {

constexpr int kCombBlock = 1024;                // the one workgroup that adds the tile triples
constexpr int kCombWaves = kCombBlock / BJX_WAVE;
constexpr double kNegInf = -__builtin_inf();

// Head of the workspace; the tile triples follow it.
struct PsHead {
  double lse;      // log-sum-exp of the log-weights (bjx_smc_persistent_weights)
  float lo, hi;    // the bracket of the bisection
  float lam;       // the temperature the next evaluation of f uses
  int32_t done;    // the whole interval was taken: the remaining launches return at once
};
constexpr int64_t kHeadBytes = 64;
static_assert(sizeof(PsHead) <= kHeadBytes, "workspace head");

// lw_j = (double)(fp32 lam * ll_j) - (double) den_j: both terms are fp32 values, so the difference is exact in fp64.
// The product, and which lw_j count, follow the weighting rule of bjx_smc_dev.h.  A term of the mixture denominator
// has the same form, with log_Z_s in the place of den_j.
__device__ __forceinline__ double ps_log_weight(float lam, float ll, float den) {
  return (double)tempered_product(lam, ll) - (double)den;
}

// persistent_sampling.py::compute_log_persistent_weights, the mixture denominator:
//   den_j = logsumexp_{s < n_terms}(lambda_s * ll_j - logZ_s) - log(n_terms)
// One thread per particle, two serial sweeps over the schedule (maximum, then sum); schedule[s] and log_Z[s] are
// uniform across the wave.  Sum in index order in fp64, rounded once.
__global__ void __launch_bounds__(kBlock)
k_ps_denominator(int64_t P, int64_t n_terms, const float* __restrict__ ll_p, const float* __restrict__ schedule,
                 const float* __restrict__ log_Z, float* __restrict__ den_out) {
  const double log_terms = log((double)n_terms);
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < P; j += (int64_t)gridDim.x * kBlock) {
    const float ll = ll_p[j];
    double m = kNegInf;
    for (int64_t s = 0; s < n_terms; ++s)
      m = fmax(m, ps_log_weight(schedule[s], ll, log_Z[s]));  // (fmax drops a NaN; the sum keeps it)
    double sum = 0.0;
    for (int64_t s = 0; s < n_terms; ++s) sum += exp(ps_log_weight(schedule[s], ll, log_Z[s]) - m);
    den_out[j] = (float)(m + log(sum) - log_terms);
  }
}

// Tile b's (max, S1, S2) of the log-weights at temperature lam, S_k relative to the tile's own maximum; a tile with
// no particle that counts writes (-inf, 0, 0).  lam is *lam_p, or comes from the bisection: lam_old + (1 - lam_old)
// at its first evaluation (`first`), head->lam afterwards.
__global__ void __launch_bounds__(kBlock)
k_ps_tile_partials(int64_t P, const float* __restrict__ ll, const float* __restrict__ den,
                   const float* __restrict__ lam_p, const float* __restrict__ lam_old_p, int first,
                   const PsHead* __restrict__ head, double* __restrict__ partials) {
  __shared__ double sh[kWavesPerBlock];
  float lam;
  if (lam_p) lam = *lam_p;
  else if (first) {
    const float lam_old = *lam_old_p;
    lam = lam_old + (1.0f - lam_old);
  } else {
    if (head->done) return;
    lam = head->lam;
  }
  const int64_t j0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kSmcItems;
  double lw[kSmcItems];
  double m = kNegInf;
#pragma unroll
  for (int e = 0; e < kSmcItems; ++e) {
    lw[e] = (j0 + e < P) ? ps_log_weight(lam, ll[j0 + e], den[j0 + e]) : kNegInf;
    if (lw_counts(lw[e])) m = fmax(m, lw[e]);
  }
  m = block_max<kWavesPerBlock>(m, sh);
  double s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int e = 0; e < kSmcItems; ++e)
    if (lw_counts(lw[e])) {
      const double x = exp(lw[e] - m);  // m = +inf: NaN, as a log-sum-exp over a +inf term is
      s1 += x;
      s2 += x * x;
    }
  s1 = block_sum<kWavesPerBlock>(s1, sh);
  s2 = block_sum<kWavesPerBlock>(s2, sh);
  if (threadIdx.x == 0) {
    double* out = partials + 3 * (int64_t)blockIdx.x;
    out[0] = m;
    out[1] = s1;
    out[2] = s2;
  }
}

// The tile triples rescaled to the overall maximum and added: M = max m_b, S_k = sum_b S_k,b exp(k (m_b - M)).  One
// workgroup of kCombBlock threads, thread t taking tiles t, t + kCombBlock, ... in order, then a fixed tree.
__device__ __forceinline__ void ps_combine(int64_t n_tiles, const double* __restrict__ partials, double* sh, double* M,
                                           double* S1, double* S2) {
  double m = kNegInf;
  for (int64_t b = threadIdx.x; b < n_tiles; b += kCombBlock) m = fmax(m, partials[3 * b]);
  m = block_max<kCombWaves>(m, sh);
  double s1 = 0.0, s2 = 0.0;
  for (int64_t b = threadIdx.x; b < n_tiles; b += kCombBlock) {
    const double mb = partials[3 * b];
    if (mb != kNegInf) {
      const double r = exp(mb - m);
      s1 += partials[3 * b + 1] * r;
      s2 += partials[3 * b + 2] * (r * r);
    }
  }
  *M = m;
  *S1 = block_sum<kCombWaves>(s1, sh);
  *S2 = block_sum<kCombWaves>(s2, sh);
}

// persistent_sampling.py::compute_log_Z: lse = logsumexp(lw), log_Z = lse - log P; -inf when no particle counts.
__global__ void __launch_bounds__(kCombBlock)
k_ps_lse(int64_t P, int64_t n_tiles, const double* __restrict__ partials, PsHead* __restrict__ head,
         float* __restrict__ log_Z_out) {
  __shared__ double sh[kCombWaves];
  double m, s1, s2;
  ps_combine(n_tiles, partials, sh, &m, &s1, &s2);
  if (threadIdx.x == 0) {
    const double lse = m == kNegInf ? kNegInf : m + log(s1);
    head->lse = lse;
    if (log_Z_out) *log_Z_out = (float)(lse - log((double)P));
  }
}

// log_weights_out = lw - lse and weights_out = exp(lw - lse), fp64, each rounded once; a particle that does not
// count has weight 0 (log-weight -inf); no particle that counts: NaN everywhere, as in k_reweight.
__global__ void __launch_bounds__(kBlock)
k_ps_write_weights(int64_t P, const float* __restrict__ ll, const float* __restrict__ den,
                   const float* __restrict__ lam_p, const PsHead* __restrict__ head, float* __restrict__ lw_out,
                   float* __restrict__ w_out) {
  const float lam = *lam_p;
  const double lse = head->lse;
  const bool none = lse == kNegInf;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < P; j += (int64_t)gridDim.x * kBlock) {
    const double lw = ps_log_weight(lam, ll[j], den[j]);
    const bool ok = lw_counts(lw);
    if (lw_out) lw_out[j] = none ? __builtin_nanf("") : (ok ? (float)(lw - lse) : -__builtin_inff());
    if (w_out) w_out[j] = none ? __builtin_nanf("") : (ok ? (float)exp(lw - lse) : 0.0f);
  }
}

// adaptive_persistent_sampling.py::calculate_lambda with solver.py::dichotomy: one step of the house bisection of
// k_ess_solve after evaluation `it` of f(delta) = log_ess(lw(lam_old + delta)) - log_target, whose tile triples the
// launch before this one wrote.  it == 0 was f(1 - lam_old): f >= 0 takes the whole interval (lam_new exactly 1) and
// marks the solve done; otherwise the bracket is [0, 1 - lam_old].  it >= 1 was f(mid): the LEFT end moves to mid
// when f(mid) >= 0 (a NaN keeps it).  After kHalvings halvings the left end is returned, so a target that no
// temperature reaches gives delta == 0 and lam_new == lam_old exactly.
__global__ void __launch_bounds__(kCombBlock)
k_ps_bracket(int64_t n_tiles, int it, double log_target, const float* __restrict__ lam_old_p,
             const double* __restrict__ partials, PsHead* __restrict__ head, float* __restrict__ delta_out,
             float* __restrict__ lam_new_out) {
  __shared__ double sh[kCombWaves];
  if (it > 0 && head->done) return;
  double m, s1, s2;
  ps_combine(n_tiles, partials, sh, &m, &s1, &s2);
  if (threadIdx.x != 0) return;
  const bool up = 2.0 * log(s1) - log(s2) - log_target >= 0.0;
  const float lam_old = *lam_old_p;
  float lo, hi;
  if (it == 0) {
    const float max_delta = 1.0f - lam_old;
    head->done = up ? 1 : 0;
    if (up) {
      *delta_out = max_delta;
      if (lam_new_out) *lam_new_out = 1.0f;
      return;
    }
    lo = 0.0f;
    hi = max_delta;
  } else {
    lo = head->lo;
    hi = head->hi;
    const float mid = 0.5f * (lo + hi);
    if (up) lo = mid;
    else hi = mid;
  }
  if (it == kHalvings) {
    *delta_out = lo;
    if (lam_new_out) *lam_new_out = lam_old + lo;
    return;
  }
  head->lo = lo;
  head->hi = hi;
  head->lam = lam_old + 0.5f * (lo + hi);
}

int64_t ps_tiles(int64_t P) { return (P + kSmcTile - 1) / kSmcTile; }

}  // namespace

extern "C" {

int bjx_smc_persistent_tile(void) { return kSmcTile; }

int64_t bjx_smc_persistent_workspace_bytes(int64_t P) {
  if (P < 1 || P > kMaxParticles) return 0;
  return kHeadBytes + ps_tiles(P) * 3 * (int64_t)sizeof(double);
}

int bjx_smc_persistent_denominator(void* stream, int64_t P, int64_t n_terms, const float* loglik,
                                   const float* schedule, const float* log_Z, float* den_out) {
  BJX_CHECK_ARG(P >= 0 && P <= kMaxParticles && n_terms >= 1 && n_terms <= kMaxParticles,
                "bjx_smc_persistent_denominator: bad sizes");
  if (P == 0) return 0;
  BJX_CHECK_ARG(loglik && schedule && log_Z && den_out, "bjx_smc_persistent_denominator: null pointer");
  hipLaunchKernelGGL(k_ps_denominator, dim3(bjx_flat_grid(P, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, P, n_terms,
                     loglik, schedule, log_Z, den_out);
  return bjx_check_launch("bjx_smc_persistent_denominator");
}

int bjx_smc_persistent_weights(void* stream, int64_t P, const float* loglik, const float* den, const float* lam,
                               void* workspace, float* log_weights_out, float* weights_out, float* log_Z_out) {
  BJX_CHECK_ARG(P >= 1 && P <= kMaxParticles, "bjx_smc_persistent_weights: bad sizes");
  BJX_CHECK_ARG(loglik && den && lam && workspace && (log_weights_out || weights_out || log_Z_out),
                "bjx_smc_persistent_weights: null pointer");
  const hipStream_t s = (hipStream_t)stream;
  PsHead* head = (PsHead*)workspace;
  double* partials = (double*)((char*)workspace + kHeadBytes);
  const int64_t nt = ps_tiles(P);
  hipLaunchKernelGGL(k_ps_tile_partials, dim3((unsigned)nt), dim3(kBlock), 0, s, P, loglik, den, lam,
                     (const float*)nullptr, 0, (const PsHead*)head, partials);
  hipLaunchKernelGGL(k_ps_lse, dim3(1), dim3(kCombBlock), 0, s, P, nt, (const double*)partials, head, log_Z_out);
  if (log_weights_out || weights_out)
    hipLaunchKernelGGL(k_ps_write_weights, dim3(bjx_flat_grid(P, kBlock)), dim3(kBlock), 0, s, P, loglik, den, lam,
                       (const PsHead*)head, log_weights_out, weights_out);
  return bjx_check_launch("bjx_smc_persistent_weights");
}

int bjx_smc_persistent_ess_solve(void* stream, int64_t P, const float* loglik, const float* den, float target,
                                 const float* lam_old, void* workspace, float* delta_out, float* lam_new_out) {
  BJX_CHECK_ARG(P >= 1 && P <= kMaxParticles && target > 0.0f && target <= (float)kMaxParticles,
                "bjx_smc_persistent_ess_solve: bad sizes");
  BJX_CHECK_ARG(loglik && den && lam_old && workspace && delta_out, "bjx_smc_persistent_ess_solve: null pointer");
  const hipStream_t s = (hipStream_t)stream;
  PsHead* head = (PsHead*)workspace;
  double* partials = (double*)((char*)workspace + kHeadBytes);
  const int64_t nt = ps_tiles(P);
  const double log_target = log((double)target);
  for (int it = 0; it <= kHalvings; ++it) {
    hipLaunchKernelGGL(k_ps_tile_partials, dim3((unsigned)nt), dim3(kBlock), 0, s, P, loglik, den,
                       (const float*)nullptr, lam_old, it == 0 ? 1 : 0, (const PsHead*)head, partials);
    hipLaunchKernelGGL(k_ps_bracket, dim3(1), dim3(kCombBlock), 0, s, nt, it, log_target, lam_old,
                       (const double*)partials, head, delta_out, lam_new_out);
  }
  return bjx_check_launch("bjx_smc_persistent_ess_solve");
}

}  // extern "C"
