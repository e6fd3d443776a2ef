// Device helpers shared by the SMC kernels (gfx950): the weighting rule, the workgroup reductions and the sizes that
// bjx_smc.hip and bjx_smc_persistent.hip must agree on.  Device code only, included by the SMC files and, for the
// workgroup and column reductions, by bjx_vi.hip.
#pragma once

#include "bjx_rows.h"

namespace bjx {

constexpr int64_t kMaxParticles = (int64_t)1 << 24;  // resampling positions are formed in fp32
constexpr int kHalvings = 30;                        // of the ESS bisection, in one kernel or across launches
constexpr int kSmcItems = 4;                         // consecutive items per thread
constexpr int kSmcTile = kBlock * kSmcItems;         // 1024 items per workgroup: the prefix scan, the persistent tiles

// The weighting rule of every SMC kernel.  A log-weight is a tempered product lam * ll (tempered.py::log_weights_fn,
// lam a temperature or a difference of two), less a denominator in persistent sampling.  lam == 0 gives a product of
// exactly 0 whatever ll is (the reference's nan_to_num of 0 * inf).  A NaN or -inf log-weight is a particle of weight
// 0 and takes no part in any maximum or sum; +inf counts.
__device__ __forceinline__ float tempered_product(float lam, float ll) { return lam == 0.0f ? 0.0f : lam * ll; }
__device__ __forceinline__ bool lw_counts(float lw) { return lw == lw && lw != -__builtin_inff(); }
__device__ __forceinline__ bool lw_counts(double lw) { return lw == lw && lw != -__builtin_inf(); }

// Sum over a workgroup of WAVES wavefronts: wave_sum, one LDS slot per wave, then the slots added in wave order.
// Every thread gets the total; sh (WAVES slots) is free again on return.
template <int WAVES>
__device__ __forceinline__ double block_sum(double v, double* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int k = 0; k < WAVES; ++k) t += sh[k];
  __syncthreads();
  return t;
}

// Column reductions of an (N, D) array (the particle moments; the gradient batch of bjx_vi.hip).  A workgroup of
// kBlock threads is cw consecutive columns (consecutive threads: reads coalesced along D) by kBlock / cw row groups.
// cw is at most 64 (one wavefront across a row piece of 256 bytes), so that wide rows spread over D / 64 workgroups per
// row tile and every column still has 4 row groups.
__host__ __device__ inline int column_block(int64_t D) { return D >= 64 ? 64 : (D >= 16 ? 16 : 4); }

// Adds the kBlock / cw row groups of a column in a fixed order; every thread of the column gets the total.  sh: kBlock
// slots, free again on return.
__device__ __forceinline__ double column_total(double v, double* sh, int cw) {
  sh[threadIdx.x] = v;
  __syncthreads();
  double t = 0.0;
  for (int k = threadIdx.x % cw; k < kBlock; k += cw) t += sh[k];
  __syncthreads();
  return t;
}

// The same for the maximum, T = float or double (exact in either; fmax drops a NaN).
template <int WAVES, typename T>
__device__ __forceinline__ T block_max(T v, T* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  T t = sh[0];
#pragma unroll
  for (int k = 1; k < WAVES; ++k) t = fmax(t, sh[k]);
  __syncthreads();
  return t;
}

}  // namespace bjx
