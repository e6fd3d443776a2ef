// Row-per-wave device helpers shared by the sampler kernels (gfx950): launch geometry, a lane's piece of a row,
// a row's normal draws, the Metropolis accept.  Device code only: also compiled by hiprtc (blackjax_amd/rtc.py).
//
// The mapping every row kernel uses.  State is (N, D) row-major fp32 and a row is a chain.  A workgroup is
// kBlock = 256 threads = kWavesPerBlock = 4 wavefronts; one wavefront owns one row at a time (wave_row0, then
// grid-stride by wave_row_stride), so everything decided per chain is wave-uniform.  The 64 lanes sweep the row in
// 16-byte pieces -- lane l holds columns 4 (l + 64 k) .. + 3 of its k-th piece (VEC = 4) -- or in 4-byte sweeps
// (VEC = 1) when D % 4 != 0 or a pointer is not 16-byte aligned (bjx_vec4_ok, BJX_LAUNCH_ROWS_VEC in bjx_host.h).
// Per-row scalars are computed by every lane and written by lane 0.
#pragma once

#include "bjx_device.h"

namespace bjx {

constexpr int kBlock = 256;  // 4 waves per workgroup
constexpr int kWavesPerBlock = kBlock / BJX_WAVE;

__device__ __forceinline__ int64_t wave_row0() {
  return (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
}
__device__ __forceinline__ int64_t wave_row_stride() { return (int64_t)gridDim.x * kWavesPerBlock; }
// The NUTS kernels' form.  The wave's index is the same in all 64 lanes: readfirstlane tells the compiler so, which
// puts everything derived from it (chain index, slot-table addresses, the threefry key arithmetic of the chain's RNG
// stream) on the scalar unit instead of repeating it in 64 vector lanes.
__device__ __forceinline__ int64_t wave_row0_uniform() {
  return (int64_t)blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

// one 16-byte (VEC = 4) or 4-byte (VEC = 1) piece of a row to / from registers
template <int VEC>
__device__ __forceinline__ void ldv(const float* p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const F4 t = ld4(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = p[0];
  }
}
template <int VEC>
__device__ __forceinline__ void stv(float* p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) st4(p, F4{v[0], v[1], v[2], v[3]});
  else p[0] = v[0];
}

// normal(key, (D,))[j .. j + VEC)
template <int VEC>
__device__ __forceinline__ void normalv(Key kn, int64_t j, float (&z)[VEC]) {
  if constexpr (VEC == 4) {
    uint32_t bits[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) bits[e] = key_bits32(kn, (uint64_t)(j + e));
    normal4_from_bits(bits, z);
  } else {
    z[0] = normal_from_bits(key_bits32(kn, (uint64_t)j));
  }
}

// proposal.py::safe_energy_diff (proposal.py:45-48): a NaN energy difference becomes -inf, so the proposal is rejected.
__device__ __forceinline__ float safe_energy_diff(float delta) {
  return delta != delta ? -__builtin_inff() : delta;
}

// proposal.py::compute_asymmetric_acceptance_ratio + static_binomial_sampling (proposal.py:214-235) on
// delta = safe_energy_diff(E(old) - E(new)): p_accept = min(exp(delta), 1) with the exp in fp64, rounded once;
// accept = uniform(key_accept) < p_accept with key_accept = split(chain key, 2)[1] of global chain `gidx`.  Every lane of
// the row's wave gets the same result.  The two steps are apart so that the HMC finishes can test divergence
// (hmc.py:162) on the patched difference between them.
__device__ __forceinline__ bool metropolis_accept(Key key, int64_t gidx, int64_t fold, float delta,
                                                  float* p_acc_out) {
  const float p_acc = fminf(exp_cr(delta), 1.0f);
  const Key kc = chain_key(key, (uint64_t)gidx, fold);
  const float u = key_uniform(key_child(kc, 1));
  *p_acc_out = p_acc;
  return u < p_acc;
}

}  // namespace bjx
