// Sequential Monte Carlo arithmetic (gfx950).  C ABI in include/bjx_hip.h ("SMC").
//
// Reference: blackjax/smc/base.py (step), smc/resampling.py (systematic, stratified: _systematic_or_stratified,
// _sorted_uniforms' callers), smc/ess.py (log_ess, ess_solver), smc/solver.py (dichotomy),
// smc/tempered.py (build_kernel: log_weights_fn, tempered_logposterior_fn); smc/resampling.py (multinomial, residual,
// _sorted_uniforms), smc/waste_free.py (update_waste_free: the layout of the kept states), smc/tuning/from_particles.py
// (particles_means, particles_stds).
//
// Resampling works on cumulative weights in 2^-62 fixed point: integer addition is associative, so the prefix sum
// is the same whatever the tiling, and the ancestor search compares integers.  The scan is launch-separated (tile
// sums -> scan of the tile sums -> apply): no workgroup ever waits on another.  The log-sum-exp reweighting and the
// ESS bisection are one workgroup each, looping over the (N,) log-likelihoods with fp64 sums: the number of
// launches does not depend on the data and nothing is read back by the host.  Which log-weights count, the order
// of a workgroup's sums and the tile of 1024 items are bjx_smc_dev.h's, shared with bjx_smc_persistent.hip.
#include <math.h>

#include "../../include/bjx_hip.h"
#include "bjx_device.h"
#include "bjx_host.h"
#include "bjx_rows.h"
#include "bjx_smc_dev.h"

using namespace bjx;

namespace {

constexpr int kRedBlock = 1024;                  // the one workgroup of the reweight / ESS kernels
constexpr int kRedWaves = kRedBlock / BJX_WAVE;
constexpr double kTwo62 = 4611686018427387904.0;

// wf = (int64) floor((double) w * 2^62); anything that is not a weight in (0, 1] is clamped so that the sum of at
// most 2^24 of them cannot leave int64 by more than a wrap the search survives (ancestors are clipped to [0, N)).
__device__ __forceinline__ int64_t scan_item(const float* in, int64_t i) {
  float w = in[i];
  if (!(w > 0.0f)) return 0;  // zero, negative, NaN
  if (w > 1.0f) w = 1.0f;
  return (int64_t)floor((double)w * kTwo62);
}
__device__ __forceinline__ int64_t scan_item(const int64_t* in, int64_t i) { return in[i]; }

// Inclusive prefix sum of one value per thread over the 256 threads of a workgroup; *total = the tile's sum.
__device__ __forceinline__ int64_t block_scan_inclusive(int64_t v, int64_t* sh, int64_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long t = __shfl_up((long long)v, o, 64);
    if (lane >= o) v += (int64_t)t;
  }
  if (lane == 63) sh[wave] = v;
  __syncthreads();
  int64_t base = 0, all = 0;
#pragma unroll
  for (int k = 0; k < kWavesPerBlock; ++k) {
    if (k < wave) base += sh[k];
    all += sh[k];
  }
  __syncthreads();
  *total = all;
  return v + base;
}

// Level 1 of the launch-separated scan: sums[b] = sum of tile b.
template <typename In>
__global__ void __launch_bounds__(kBlock) k_tile_sums(const In* in, int64_t n, int64_t* sums) {
  __shared__ int64_t sh[kWavesPerBlock];
  const int64_t i0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kSmcItems;
  int64_t s = 0;
#pragma unroll
  for (int e = 0; e < kSmcItems; ++e)
    if (i0 + e < n) s += scan_item(in, i0 + e);
  int64_t total;
  block_scan_inclusive(s, sh, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// Level 3: out[i] = tile_offsets[b - 1] + inclusive prefix inside tile b.  `tile_offsets` (null for a single tile)
// holds the INCLUSIVE scan of the tile sums.  A thread reads only the items it writes, so in == out is allowed.
template <typename In>
__global__ void __launch_bounds__(kBlock) k_tile_scan(const In* in, int64_t n, const int64_t* tile_offsets,
                                                      int64_t* out) {
  __shared__ int64_t sh[kWavesPerBlock];
  const int64_t i0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kSmcItems;
  int64_t v[kSmcItems];
  int64_t s = 0;
#pragma unroll
  for (int e = 0; e < kSmcItems; ++e) {
    v[e] = (i0 + e < n) ? scan_item(in, i0 + e) : 0;
    s += v[e];
    v[e] = s;
  }
  int64_t total;
  const int64_t incl = block_scan_inclusive(s, sh, &total);
  const int64_t base = (incl - s) + ((tile_offsets && blockIdx.x > 0) ? tile_offsets[blockIdx.x - 1] : 0);
#pragma unroll
  for (int e = 0; e < kSmcItems; ++e)
    if (i0 + e < n) out[i0 + e] = base + v[e];
}

// #{j < N : c_j < t}
__device__ __forceinline__ int64_t count_below(const int64_t* __restrict__ c, int64_t N, int64_t t) {
  int64_t lo = 0, hi = N;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (c[mid] < t) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// min(N - 1, #{j : c_j < t}): searchsorted(c, t) and the reference's clip, so an ancestor is always in [0, N)
__device__ __forceinline__ int32_t ancestor_below(const int64_t* __restrict__ c, int64_t N, int64_t t) {
  const int64_t a = count_below(c, N, t);
  return (int32_t)(a < N - 1 ? a : N - 1);
}

// resampling.py::systematic / stratified: pos_i = (i + u_i) / M in fp32, u_i = uniform(key, ()) for every i
// (systematic) or uniform(key, (M,))[i] (stratified); ancestor_i = min(N - 1, #{j : C_j < t_i}) with
// t_i = (int64)(pos_i * 2^62), exact in fp64 -- searchsorted(cumsum(w), pos) and the reference's clip.
template <bool STRATIFIED>
__global__ void __launch_bounds__(kBlock)
k_resample(Key key, int64_t N, int64_t M, const int64_t* __restrict__ cum, int32_t* __restrict__ ancestors) {
  const float u_sys = key_uniform(key);
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < M; i += (int64_t)gridDim.x * kBlock) {
    const float u = STRATIFIED ? fmaxf(0.0f, unit_float(key_bits32(key, (uint64_t)i))) : u_sys;
    const float pos = ((float)i + u) / (float)M;
    ancestors[i] = ancestor_below(cum, N, (int64_t)((double)pos * kTwo62));
  }
}

// One row copied by the row's wavefront, 16 bytes (VEC = 4) or 4 bytes per lane
template <int VEC>
__device__ __forceinline__ void copy_row(float* __restrict__ dst, const float* __restrict__ src, int64_t D) {
  for (int64_t j = (int64_t)(threadIdx.x & 63) * VEC; j < D; j += 64 * VEC) {
    if constexpr (VEC == 4) st4(dst + j, ld4(src + j));
    else dst[j] = src[j];
  }
}

// out[i, :] = x[ancestors[i], :], one wavefront per output row.  An index outside [0, N) is clamped: the launch
// stays inside x whatever it is given.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_gather(int64_t N, int64_t M, int64_t D, const float* __restrict__ x, const int32_t* __restrict__ ancestors,
         float* __restrict__ out) {
  for (int64_t r = wave_row0(); r < M; r += wave_row_stride()) {
    int64_t a = ancestors[r];
    a = a < 0 ? 0 : (a > N - 1 ? N - 1 : a);
    copy_row<VEC>(out + r * D, x + a * D, D);
  }
}

// tempered.py::tempered_logposterior_fn and its gradient: lp + lam * ll and gp + lam * gl, the product rounded
// before the sum (no fmaf: NumPy reproduces both bit for bit).
__device__ __forceinline__ float tempered_sum(float p, float lam, float l) {
  const float t = lam * l;
  return p + t;
}

// lp_out = lp + lam * ll over (N,), grid-stride: the one form of the value, so a value-only sampler (random walk)
// and a gradient sampler see the same tempered log-density bit for bit
__device__ __forceinline__ void temper_values(int64_t N, float lam, const float* __restrict__ lp,
                                              const float* __restrict__ ll, float* __restrict__ lp_out) {
  const int64_t nthr = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < N; i += nthr)
    lp_out[i] = tempered_sum(lp[i], lam, ll[i]);
}

// Value and gradient.  lam is read from device memory, so one recorded or traced launch serves every temperature.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_temper(int64_t N, int64_t D, const float* __restrict__ lam_p, const float* __restrict__ lp,
         const float* __restrict__ gp, const float* __restrict__ ll, const float* __restrict__ gl,
         float* __restrict__ lp_out, float* __restrict__ g_out) {
  const float lam = *lam_p;
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x, nthr = (int64_t)gridDim.x * kBlock;
  const int64_t total = N * D;
  for (int64_t i = tid * VEC; i < total; i += nthr * VEC) {
    if constexpr (VEC == 4) {
      const F4 a = ld4(gp + i), b = ld4(gl + i);
      st4(g_out + i, F4{tempered_sum(a.x, lam, b.x), tempered_sum(a.y, lam, b.y), tempered_sum(a.z, lam, b.z),
                        tempered_sum(a.w, lam, b.w)});
    } else {
      g_out[i] = tempered_sum(gp[i], lam, gl[i]);
    }
  }
  temper_values(N, lam, lp, ll, lp_out);
}

// The value alone
__global__ void __launch_bounds__(kBlock)
k_temper_value(int64_t N, const float* __restrict__ lam_p, const float* __restrict__ lp,
               const float* __restrict__ ll, float* __restrict__ lp_out) {
  temper_values(N, *lam_p, lp, ll, lp_out);
}

// ---- one-workgroup reductions over (N,) -------------------------------------------------------------------
// lw(j) is the log-weight of item j; which entries count, and the order of the sums, are bjx_smc_dev.h's.
// The maximum over the entries that count; -inf when none does.
template <class LogWeight>
__device__ __forceinline__ float max_counted(int64_t N, LogWeight lw, float* sh) {
  float m = -__builtin_inff();
  for (int64_t j = threadIdx.x; j < N; j += kRedBlock) {
    const float v = lw(j);
    if (lw_counts(v)) m = fmaxf(m, v);
  }
  return block_max<kRedWaves>(m, sh);
}

// S_k = sum exp(k (lw - m)) over the entries that count, k = 1, 2; the exponential and the sums in fp64.
template <class LogWeight>
__device__ __forceinline__ void sums_against(int64_t N, LogWeight lw, float m, double* sh, double* S1, double* S2) {
  double s1 = 0.0, s2 = 0.0;
  for (int64_t j = threadIdx.x; j < N; j += kRedBlock) {
    const float v = lw(j);
    if (lw_counts(v)) {
      const double e = exp((double)v - (double)m);
      s1 += e;
      s2 += e * e;
    }
  }
  *S1 = block_sum<kRedWaves>(s1, sh);
  *S2 = block_sum<kRedWaves>(s2, sh);
}

// base.py::step, the weighting: lw = (lam_new - lam_old) * ll ; lse = logsumexp(lw) ; w = exp(lw - lse) ;
// log_likelihood_increment = lse - log N.  exp and log in fp64, the sum in fp64, each result rounded once.
__global__ void __launch_bounds__(kRedBlock)
k_reweight(int64_t N, const float* __restrict__ ll, const float* __restrict__ lam_old_p,
           const float* __restrict__ lam_new_p, float* __restrict__ w_out, float* __restrict__ inc_out,
           float* __restrict__ lam_out) {
  __shared__ double shd[kRedWaves];
  __shared__ float shf[kRedWaves];
  const float lam_new = *lam_new_p;
  const float delta = lam_new - *lam_old_p;
  const auto lw_of = [&](int64_t j) { return tempered_product(delta, ll[j]); };
  const float m = max_counted(N, lw_of, shf);
  double s = 0.0;  // S1 alone: the shared sweep would add S2's multiply
  for (int64_t j = threadIdx.x; j < N; j += kRedBlock) {
    const float lw = lw_of(j);
    if (lw_counts(lw)) s += exp((double)lw - (double)m);
  }
  s = block_sum<kRedWaves>(s, shd);
  const bool none = m == -__builtin_inff();  // no particle of positive weight: weights NaN, increment -inf
  const double lse = none ? -(double)__builtin_inff() : (double)m + log(s);
  for (int64_t j = threadIdx.x; j < N; j += kRedBlock) {
    const float lw = lw_of(j);
    w_out[j] = none ? __builtin_nanf("") : (lw_counts(lw) ? (float)exp((double)lw - lse) : 0.0f);
  }
  if (threadIdx.x == 0) {
    *inc_out = (float)(lse - log((double)N));
    *lam_out = lam_new;
  }
}

// ess.py::log_ess = 2 logsumexp(lw) - logsumexp(2 lw) = 2 log S1 - log S2 with S_k = sum exp(k (lw - max)).
__global__ void __launch_bounds__(kRedBlock)
k_log_ess(int64_t N, const float* __restrict__ lw_in, float* __restrict__ out) {
  __shared__ double shd[kRedWaves];
  __shared__ float shf[kRedWaves];
  const auto lw_of = [&](int64_t j) { return lw_in[j]; };
  double s1, s2;
  sums_against(N, lw_of, max_counted(N, lw_of, shf), shd, &s1, &s2);
  if (threadIdx.x == 0) *out = (float)(2.0 * log(s1) - log(s2));
}

// ess.py::ess_solver with solver.py::dichotomy, entirely on the device: f(d) = log_ess(d * ll) - log(N target).
// f(max_delta) >= 0: delta = max_delta (and lam_new exactly 1 when max_delta is 1 - lam_old).  Otherwise 30
// halvings of [0, max_delta] in fp32 that move the LEFT end to mid whenever f(mid) >= 0 and return the left end:
// the ESS at the returned delta is never below the target.  max(d * ll) = d * max(ll) for d >= 0 (rounding is
// monotone), so every evaluation of f is one sweep: e = exp(d * ll - d * ll_max) per particle in fp64 (an fp32
// exponential would blur f by 1e-7, a hundred bisection widths), summed (and squared and summed) in fp64.
__global__ void __launch_bounds__(kRedBlock)
k_ess_solve(int64_t N, const float* __restrict__ ll, double log_target, const float* __restrict__ max_delta_p,
            const float* __restrict__ lam_old_p, float* __restrict__ delta_out, float* __restrict__ lam_new_out) {
  __shared__ double shd[kRedWaves];
  __shared__ float shf[kRedWaves];
  const float lam_old = lam_old_p ? *lam_old_p : 0.0f;
  const float max_delta = max_delta_p ? *max_delta_p : 1.0f - lam_old;
  const float ll_max = max_counted(N, [&](int64_t j) { return ll[j]; }, shf);

  auto f = [&](float d) -> double {
    double s1, s2;
    sums_against(N, [&](int64_t j) { return tempered_product(d, ll[j]); }, tempered_product(d, ll_max), shd, &s1, &s2);
    return 2.0 * log(s1) - log(s2) - log_target;
  };

  float delta;
  bool full = false;
  if (f(max_delta) >= 0.0) {
    delta = max_delta;
    full = true;
  } else {
    float lo = 0.0f, hi = max_delta;
    for (int it = 0; it < kHalvings; ++it) {
      const float mid = 0.5f * (lo + hi);
      if (f(mid) >= 0.0) lo = mid;  // (a NaN keeps the left end)
      else hi = mid;
    }
    delta = lo;
  }
  if (threadIdx.x == 0) {
    *delta_out = delta;
    if (lam_new_out) *lam_new_out = (full && !max_delta_p) ? 1.0f : lam_old + delta;
  }
}

// ---- multinomial / residual resampling: sorted uniforms from an integer prefix sum of exponentials ----------
constexpr double kTwo24 = 16777216.0;
constexpr uint64_t kMask62 = ((uint64_t)1 << 62) - 1;

// resampling.py::_sorted_uniforms, the exponentials: ef_k = (int64) floor((double) e_k * 2^24) with
// e_k = -log1p(-u_k) correctly rounded to fp32 and u_k = uniform(key, (count,))[k].  e_k < 16, so the sum of
// 2^24 + 1 of them stays below 2^53.
__global__ void __launch_bounds__(kBlock) k_exp_fixed(Key key, int64_t count, int64_t* __restrict__ ef) {
  for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < count; k += (int64_t)gridDim.x * kBlock) {
    const float u = fmaxf(0.0f, unit_float(key_bits32(key, (uint64_t)k)));
    const float e = bjx_neg_log1p(-u);
    ef[k] = (int64_t)floor((double)e * kTwo24);
  }
}

// pos_i = Z_i / max(Z_M, 1) in fp64 (both conversions exact, the division rounded once): the i-th sorted uniform
__device__ __forceinline__ double sorted_uniform(const int64_t* __restrict__ z, int64_t M, int64_t i) {
  const int64_t zm = z[M];
  return (double)z[i] / (double)(zm > 1 ? zm : 1);
}

// resampling.py::multinomial: ancestor_i = min(N - 1, #{j : C_j < (int64)(pos_i * 2^62)})
__global__ void __launch_bounds__(kBlock)
k_resample_multinomial(int64_t N, int64_t M, const int64_t* __restrict__ cum, const int64_t* __restrict__ z,
                       int32_t* __restrict__ ancestors) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < M; i += (int64_t)gridDim.x * kBlock)
    ancestors[i] = ancestor_below(cum, N, (int64_t)(sorted_uniform(z, M, i) * kTwo62));
}

// resampling.py::residual, the split: prod_j = wf_j * M exactly (at most 86 bits), cnt_j = prod_j >> 62 copies for
// certain, rem_j = (prod_j mod 2^62) >> 24 the weight of particle j in the multinomial draw of the rest.
__global__ void __launch_bounds__(kBlock)
k_residual_split(int64_t N, int64_t M, const float* __restrict__ w, int64_t* __restrict__ cnt,
                 int64_t* __restrict__ rem) {
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < N; j += (int64_t)gridDim.x * kBlock) {
    const uint64_t wf = (uint64_t)scan_item(w, j);
    const uint64_t lo = wf * (uint64_t)M, hi = __umul64hi(wf, (uint64_t)M);
    cnt[j] = (int64_t)((hi << 2) | (lo >> 62));
    rem[j] = (int64_t)((lo & kMask62) >> 24);
  }
}

// Position i < S = Ccnt[N - 1] is the i-th entry of repeat(arange(N), cnt): #{j : Ccnt_j <= i}.  Position i >= S is
// entry perm[i] of the multinomial sample of the remainders: min(N - 1, #{j : Crem_j < (int64)(pos_p * Crem[N - 1])}).
__global__ void __launch_bounds__(kBlock)
k_resample_residual(int64_t N, int64_t M, const int64_t* __restrict__ ccnt, const int64_t* __restrict__ crem,
                    const int64_t* __restrict__ z, const int32_t* __restrict__ perm,
                    int32_t* __restrict__ ancestors) {
  const int64_t S = ccnt[N - 1];
  const double rem_total = (double)crem[N - 1];
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < M; i += (int64_t)gridDim.x * kBlock) {
    if (i < S) {
      ancestors[i] = ancestor_below(ccnt, N, i + 1);
    } else {
      int64_t p = perm ? (int64_t)perm[i] : i;
      p = p < 0 ? 0 : (p > M - 1 ? M - 1 : p);  // the read of z stays in bounds whatever perm holds
      ancestors[i] = ancestor_below(crem, N, (int64_t)(sorted_uniform(z, M, p) * rem_total));
    }
  }
}

// out[row0 + i * row_stride, :] = x[i, :], one wavefront per source row (the mapping of k_gather)
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_scatter_rows(int64_t M, int64_t D, const float* __restrict__ x, int64_t row0, int64_t row_stride,
               float* __restrict__ out) {
  for (int64_t r = wave_row0(); r < M; r += wave_row_stride())
    copy_row<VEC>(out + (row0 + r * row_stride) * D, x + r * D, D);
}

// ---- column moments of the particles -----------------------------------------------------------------------
constexpr int kMomTile = 256;  // rows per workgroup: fixed, so the partials depend on (N, D) alone

// Workgroup (tile, column block): cw consecutive columns (consecutive threads: reads coalesced along D) by
// kBlock / cw row groups.  part[(tile * D + j) * 2 + {0, 1}] = the tile's mean of column j and its sum of squared
// deviations from that mean, fp64.
__global__ void __launch_bounds__(kBlock)
k_moments_tile(int64_t N, int64_t D, int cw, const float* __restrict__ x, double* __restrict__ part) {
  __shared__ double sh[kBlock];
  const int tx = threadIdx.x % cw, ty = threadIdx.x / cw, groups = kBlock / cw;
  const int64_t j = (int64_t)blockIdx.y * cw + tx;
  const int64_t r0 = (int64_t)blockIdx.x * kMomTile;
  const int64_t r1 = r0 + kMomTile < N ? r0 + kMomTile : N;
  double s = 0.0;
  if (j < D)
    for (int64_t r = r0 + ty; r < r1; r += groups) s += (double)x[r * D + j];
  const double mean = column_total(s, sh, cw) / (double)(r1 - r0);
  double q = 0.0;
  if (j < D)
    for (int64_t r = r0 + ty; r < r1; r += groups) {
      const double d = (double)x[r * D + j] - mean;
      q += d * d;
    }
  q = column_total(q, sh, cw);
  if (ty == 0 && j < D) {
    part[(blockIdx.x * D + j) * 2] = mean;
    part[(blockIdx.x * D + j) * 2 + 1] = q;
  }
}

// One thread per column merges the tiles in order (Chan et al.): mean and M2 of the union of two sets.  The fp64
// results stay in `total` (mean (D,), then M2 (D,)) for callers that centre the rows.
__global__ void __launch_bounds__(kBlock)
k_moments_combine(int64_t N, int64_t D, int64_t tiles, const double* __restrict__ part, double* __restrict__ total,
                  float* __restrict__ mean_out, float* __restrict__ std_out) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= D) return;
  double n = 0.0, mean = 0.0, m2 = 0.0;
  for (int64_t t = 0; t < tiles; ++t) {
    const int64_t r0 = t * kMomTile;
    const double nb = (double)((r0 + kMomTile < N ? r0 + kMomTile : N) - r0);
    const double delta = part[(t * D + j) * 2] - mean, nn = n + nb;
    mean += delta * (nb / nn);
    m2 += part[(t * D + j) * 2 + 1] + delta * delta * (n * nb / nn);
    n = nn;
  }
  total[j] = mean;
  total[D + j] = m2;
  mean_out[j] = (float)mean;
  if (std_out) std_out[j] = (float)sqrt(m2 / (double)N);
}

int64_t n_tiles(int64_t n) { return (n + kSmcTile - 1) / kSmcTile; }

// int64 words of an n-item scan: the items, then the tile sums of every level
int64_t scan_words(int64_t n) {
  int64_t words = n;
  for (int64_t m = n; n_tiles(m) > 1; m = n_tiles(m)) words += n_tiles(m);
  return words;
}

constexpr int64_t kMaxMomentCols = (int64_t)1 << 20;
int64_t mom_tiles(int64_t N) { return (N + kMomTile - 1) / kMomTile; }

// Inclusive scan of n items into out; ws holds the tile sums of this level and of every level above it.
template <typename In>
void scan_level(hipStream_t stream, const In* in, int64_t n, int64_t* out, int64_t* ws) {
  const int64_t nt = n_tiles(n);
  if (nt == 1) {
    hipLaunchKernelGGL(k_tile_scan<In>, dim3(1), dim3(kBlock), 0, stream, in, n, (const int64_t*)nullptr, out);
    return;
  }
  hipLaunchKernelGGL(k_tile_sums<In>, dim3((unsigned)nt), dim3(kBlock), 0, stream, in, n, ws);
  scan_level<int64_t>(stream, ws, nt, ws, ws + nt);
  hipLaunchKernelGGL(k_tile_scan<In>, dim3((unsigned)nt), dim3(kBlock), 0, stream, in, n, (const int64_t*)ws, out);
}

}  // namespace

extern "C" {

int bjx_smc_scan_tile(void) { return kSmcTile; }

int64_t bjx_smc_resample_workspace_bytes(int64_t N) {
  if (N < 1 || N > kMaxParticles) return 0;
  return scan_words(N) * (int64_t)sizeof(int64_t);  // the cumulative weights, then the tile sums of every level
}

int bjx_smc_resample(void* stream, uint32_t key0, uint32_t key1, int32_t stratified, int64_t N,
                     int64_t num_samples, const float* weights, int64_t* workspace, int32_t* ancestors_out) {
  BJX_CHECK_ARG(N >= 1 && N <= kMaxParticles && num_samples >= 0 && num_samples <= kMaxParticles,
                "bjx_smc_resample: bad sizes");
  if (num_samples == 0) return 0;
  BJX_CHECK_ARG(weights && workspace && ancestors_out, "bjx_smc_resample: null pointer");
  const hipStream_t s = (hipStream_t)stream;
  scan_level<float>(s, weights, N, workspace, workspace + N);
  const Key key{key0, key1};
  const dim3 grid(bjx_flat_grid(num_samples, kBlock)), block(kBlock);
  if (stratified)
    hipLaunchKernelGGL(k_resample<true>, grid, block, 0, s, key, N, num_samples, (const int64_t*)workspace,
                       ancestors_out);
  else
    hipLaunchKernelGGL(k_resample<false>, grid, block, 0, s, key, N, num_samples, (const int64_t*)workspace,
                       ancestors_out);
  return bjx_check_launch("bjx_smc_resample");
}

int64_t bjx_smc_resample_sorted_workspace_bytes(int64_t N, int64_t num_samples) {
  if (N < 1 || N > kMaxParticles || num_samples < 0 || num_samples > kMaxParticles) return 0;
  // two scans over the particles (cumulative weights, or copies and remainders), one over the exponentials
  return (2 * scan_words(N) + scan_words(num_samples + 1)) * (int64_t)sizeof(int64_t);
}

int bjx_smc_resample_sorted(void* stream, uint32_t key0, uint32_t key1, int32_t mode, int64_t N,
                            int64_t num_samples, const float* weights, const int32_t* perm, int64_t* workspace,
                            int32_t* ancestors_out) {
  BJX_CHECK_ARG(N >= 1 && N <= kMaxParticles && num_samples >= 0 && num_samples <= kMaxParticles &&
                    (mode == BJX_SMC_MULTINOMIAL || mode == BJX_SMC_RESIDUAL),
                "bjx_smc_resample_sorted: bad sizes");
  if (num_samples == 0) return 0;
  BJX_CHECK_ARG(weights && workspace && ancestors_out, "bjx_smc_resample_sorted: null pointer");
  const hipStream_t s = (hipStream_t)stream;
  const int64_t M = num_samples, wn = scan_words(N);
  int64_t* a = workspace;           // C, or Ccnt
  int64_t* b = workspace + wn;      // Crem
  int64_t* z = workspace + 2 * wn;  // Z, M + 1 items
  const dim3 block(kBlock);
  hipLaunchKernelGGL(k_exp_fixed, dim3(bjx_flat_grid(M + 1, kBlock)), block, 0, s, Key{key0, key1}, M + 1, z);
  scan_level<int64_t>(s, z, M + 1, z, z + M + 1);
  if (mode == BJX_SMC_MULTINOMIAL) {
    scan_level<float>(s, weights, N, a, a + N);
    hipLaunchKernelGGL(k_resample_multinomial, dim3(bjx_flat_grid(M, kBlock)), block, 0, s, N, M, (const int64_t*)a,
                       (const int64_t*)z, ancestors_out);
  } else {
    hipLaunchKernelGGL(k_residual_split, dim3(bjx_flat_grid(N, kBlock)), block, 0, s, N, M, weights, a, b);
    scan_level<int64_t>(s, a, N, a, a + N);
    scan_level<int64_t>(s, b, N, b, b + N);
    hipLaunchKernelGGL(k_resample_residual, dim3(bjx_flat_grid(M, kBlock)), block, 0, s, N, M, (const int64_t*)a,
                       (const int64_t*)b, (const int64_t*)z, perm, ancestors_out);
  }
  return bjx_check_launch("bjx_smc_resample_sorted");
}

int bjx_smc_scatter_rows(void* stream, int64_t M, int64_t D, const float* x, int64_t row0, int64_t row_stride,
                         float* out) {
  BJX_CHECK_ARG(M >= 0 && D > 0 && row0 >= 0 && row_stride >= 1, "bjx_smc_scatter_rows: bad sizes");
  if (M == 0) return 0;
  BJX_CHECK_ARG(x && out, "bjx_smc_scatter_rows: null pointer");
  BJX_CHECK_ARG(x != out, "bjx_smc_scatter_rows: out of place only");
  BJX_LAUNCH_ROWS_VEC(bjx_vec4_ok(D, x, out), k_scatter_rows, M, stream, M, D, x, row0, row_stride, out);
  return bjx_check_launch("bjx_smc_scatter_rows");
}

int bjx_smc_moments_tile(void) { return kMomTile; }

int64_t bjx_smc_particle_moments_workspace_bytes(int64_t N, int64_t D) {
  if (N < 1 || N > kMaxParticles || D < 1 || D > kMaxMomentCols) return 0;
  return (2 * mom_tiles(N) * D + 2 * D) * (int64_t)sizeof(double);  // the tiles' partials, then mean and M2
}

int bjx_smc_particle_moments(void* stream, int64_t N, int64_t D, const float* x, void* workspace, float* mean_out,
                             float* std_out) {
  BJX_CHECK_ARG(N >= 1 && N <= kMaxParticles && D >= 1 && D <= kMaxMomentCols,
                "bjx_smc_particle_moments: bad sizes");
  BJX_CHECK_ARG(x && workspace && mean_out, "bjx_smc_particle_moments: null pointer");
  const int64_t tiles = mom_tiles(N);
  const int cw = column_block(D);
  double* part = (double*)workspace;
  hipLaunchKernelGGL(k_moments_tile, dim3((unsigned)tiles, (unsigned)((D + cw - 1) / cw)), dim3(kBlock), 0,
                     (hipStream_t)stream, N, D, cw, x, part);
  hipLaunchKernelGGL(k_moments_combine, dim3(bjx_flat_grid(D, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, N, D,
                     tiles, (const double*)part, part + 2 * tiles * D, mean_out, std_out);
  return bjx_check_launch("bjx_smc_particle_moments");
}

int bjx_smc_gather(void* stream, int64_t N, int64_t num_samples, int64_t D, const float* x,
                   const int32_t* ancestors, float* out) {
  BJX_CHECK_ARG(N >= 1 && num_samples >= 0 && D > 0, "bjx_smc_gather: bad sizes");
  if (num_samples == 0) return 0;
  BJX_CHECK_ARG(x && ancestors && out, "bjx_smc_gather: null pointer");
  BJX_CHECK_ARG(x != out, "bjx_smc_gather: out of place only");
  BJX_LAUNCH_ROWS_VEC(bjx_vec4_ok(D, x, out), k_gather, num_samples, stream, N, num_samples, D, x, ancestors, out);
  return bjx_check_launch("bjx_smc_gather");
}

int bjx_smc_temper(void* stream, int64_t N, int64_t D, const float* lam, const float* logprior,
                   const float* logprior_grad, const float* loglik, const float* loglik_grad, float* logp_out,
                   float* grad_out) {
  BJX_CHECK_ARG(N >= 0 && D > 0, "bjx_smc_temper: bad sizes");
  if (N == 0) return 0;
  BJX_CHECK_ARG(lam && logprior && logprior_grad && loglik && loglik_grad && logp_out && grad_out,
                "bjx_smc_temper: null pointer");
  const dim3 block(kBlock);
  if (bjx_vec4_ok(D, logprior_grad, loglik_grad, grad_out))
    hipLaunchKernelGGL(k_temper<4>, dim3(bjx_flat_grid(N * D / 4, kBlock)), block, 0, (hipStream_t)stream, N, D, lam,
                       logprior, logprior_grad, loglik, loglik_grad, logp_out, grad_out);
  else
    hipLaunchKernelGGL(k_temper<1>, dim3(bjx_flat_grid(N * D, kBlock)), block, 0, (hipStream_t)stream, N, D, lam,
                       logprior, logprior_grad, loglik, loglik_grad, logp_out, grad_out);
  return bjx_check_launch("bjx_smc_temper");
}

int bjx_smc_temper_value(void* stream, int64_t N, const float* lam, const float* logprior, const float* loglik,
                         float* logp_out) {
  BJX_CHECK_ARG(N >= 0, "bjx_smc_temper_value: bad sizes");
  if (N == 0) return 0;
  BJX_CHECK_ARG(lam && logprior && loglik && logp_out, "bjx_smc_temper_value: null pointer");
  hipLaunchKernelGGL(k_temper_value, dim3(bjx_flat_grid(N, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, N, lam,
                     logprior, loglik, logp_out);
  return bjx_check_launch("bjx_smc_temper_value");
}

int bjx_smc_reweight(void* stream, int64_t N, const float* loglik, const float* lam_old, const float* lam_new,
                     float* weights_out, float* log_likelihood_increment_out, float* lam_out) {
  BJX_CHECK_ARG(N >= 1, "bjx_smc_reweight: bad sizes");
  BJX_CHECK_ARG(loglik && lam_old && lam_new && weights_out && log_likelihood_increment_out && lam_out,
                "bjx_smc_reweight: null pointer");
  hipLaunchKernelGGL(k_reweight, dim3(1), dim3(kRedBlock), 0, (hipStream_t)stream, N, loglik, lam_old, lam_new,
                     weights_out, log_likelihood_increment_out, lam_out);
  return bjx_check_launch("bjx_smc_reweight");
}

int bjx_smc_log_ess(void* stream, int64_t N, const float* log_weights, float* log_ess_out) {
  BJX_CHECK_ARG(N >= 1, "bjx_smc_log_ess: bad sizes");
  BJX_CHECK_ARG(log_weights && log_ess_out, "bjx_smc_log_ess: null pointer");
  hipLaunchKernelGGL(k_log_ess, dim3(1), dim3(kRedBlock), 0, (hipStream_t)stream, N, log_weights, log_ess_out);
  return bjx_check_launch("bjx_smc_log_ess");
}

int bjx_smc_ess_solve(void* stream, int64_t N, const float* loglik, float target_ess, const float* max_delta,
                      const float* lam_old, float* delta_out, float* lam_new_out) {
  BJX_CHECK_ARG(N >= 1 && target_ess > 0.0f && target_ess <= 1.0f, "bjx_smc_ess_solve: bad sizes");
  BJX_CHECK_ARG(loglik && (max_delta || lam_old) && delta_out, "bjx_smc_ess_solve: null pointer");
  const double log_target = log((double)N * (double)target_ess);
  hipLaunchKernelGGL(k_ess_solve, dim3(1), dim3(kRedBlock), 0, (hipStream_t)stream, N, loglik, log_target,
                     max_delta, lam_old, delta_out, lam_new_out);
  return bjx_check_launch("bjx_smc_ess_solve");
}

}  // extern "C"
