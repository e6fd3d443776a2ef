// The accept-and-select finish of a transition (gfx950), shared by the samplers whose finish is: sum one or two
// per-element terms over the row in fp64, turn the sums and the two log-densities into an energy difference, draw the
// Metropolis accept, write the per-chain scalars and copy the chosen state out of place.  bjx_mala.hip, bjx_barker.hip
// and bjx_mgrad.hip instantiate it.  Device code; layout and mapping: bjx_rows.h.
//
// A state is a row pair: a (position) and b (gradient), index 0 the current state, 1 the proposal.  A sampler supplies
// a policy T, passed by value as the kernel argument after D, where the samplers' own kernels had their step size:
//   struct Row; Row row(int64_t r) const   the per-row scalars (a per-chain step size and what derives from it)
//   static constexpr int kSums             the number of fp64 sums, 1 or 2 (with 1, s1 is left alone)
//   static void term(row, aux, a0, a1, b0, b1, double& s0, double& s1)   adds one element's terms to the sums
//   static float delta(row, s0, s1, lp0, lp1)   from the wave-summed s0, s1 and the two log-densities, the argument
//                                          of metropolis_accept: safe_energy_diff already applied
//   static constexpr bool kAux             the term also reads aux[j] of a (D,) operand shared by all rows, and the
//                                          launch may carry a second row pair c, d (c_out non-null), selected by the
//                                          same accept flag and read once, from the chosen source.  When false, aux,
//                                          c0, d0, c1, d1, c_out and d_out are not looked at: pass nullptr.
// The accept key is split(chain key, 2)[1] of global chain r + off (metropolis_accept).  Outputs do not alias inputs.
// Two things here are as they are for the compiler's sake (NOTEBOOK.md section 25): the sums are two scalars, not a
// double[kSums], and the kAux-only pointers come last in the argument list, so that the arguments a policy without
// them uses are laid out as they were in its own kernel.  They are kernel arguments, not policy members, because the
// copy of the carried pair needs them __restrict__.
//
// Two forms, chosen by BJX_LAUNCH_ROWS_RES (bjx_host.h):
//   k_finish_res<NI>  16-byte rows of at most 256 * NI floats.  a0, a1, b0, b1 stay in registers between the reduction
//                     and the select: 16 B read + 8 B written = 24 B per element, nothing re-read.
//   k_finish<VEC>     any row.  Pass 1 sweeps the four rows once, pass 2 reads the chosen pair again (wave-uniform
//                     source rows): 32 B per element.
// A carried pair adds 8 B read + 8 B written = 16 B per element to either form.  aux is served from cache.
//
// VGPRs (kernel-resource-usage remark of the gfx950 build), no scratch anywhere:
//                      k_finish_res<1> / <2> / <4>    k_finish<4> / <1>
//   mala   (2 sums)        66 /  71 / 105                 70 / 62
//   barker (1 sum)         87 /  94 / 127                101 / 84
//   mgrad  (2 sums, aux)   75 /  78 / 110                 88 / 71
#pragma once

#include "bjx_rows.h"

namespace bjx {

template <int VEC, class T>
__global__ void __launch_bounds__(kBlock)
k_finish(Key key, int64_t off, int64_t fold, int64_t N, int64_t D, T pol, const float* __restrict__ a0,
         const float* __restrict__ logp0, const float* __restrict__ b0, const float* __restrict__ a1,
         const float* __restrict__ logp1, const float* __restrict__ b1, float* __restrict__ a_out,
         float* __restrict__ logp_out, float* __restrict__ b_out, float* __restrict__ acc_rate_out,
         uint8_t* __restrict__ is_acc_out, const float* __restrict__ aux, const float* __restrict__ c0,
         const float* __restrict__ d0, const float* __restrict__ c1, const float* __restrict__ d1,
         float* __restrict__ c_out, float* __restrict__ d_out) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = wave_row0(); r < N; r += wave_row_stride()) {
    const typename T::Row row = pol.row(r);
    const int64_t base = r * D;
    double s0 = 0.0, s1 = 0.0;
    for (int64_t j = (int64_t)lane * VEC; j < D; j += 64 * VEC) {
      float x0[VEC], x1[VEC], y0[VEC], y1[VEC], ax[VEC] = {};
      ldv<VEC>(a0 + base + j, x0);
      ldv<VEC>(a1 + base + j, x1);
      ldv<VEC>(b0 + base + j, y0);
      ldv<VEC>(b1 + base + j, y1);
      if constexpr (T::kAux) ldv<VEC>(aux + j, ax);
#pragma unroll
      for (int e = 0; e < VEC; ++e) T::term(row, ax[e], x0[e], x1[e], y0[e], y1[e], s0, s1);
    }
    s0 = wave_sum(s0);
    if constexpr (T::kSums == 2) s1 = wave_sum(s1);
    const float lp0 = logp0[r], lp1 = logp1[r];
    float p_acc;
    const bool accept = metropolis_accept(key, r + off, fold, T::delta(row, s0, s1, lp0, lp1), &p_acc);
    if (lane == 0) {
      acc_rate_out[r] = p_acc;
      is_acc_out[r] = accept ? 1 : 0;
      logp_out[r] = accept ? lp1 : lp0;
    }
    const float* as = accept ? a1 : a0;
    const float* bs = accept ? b1 : b0;
    for (int64_t j = (int64_t)lane * VEC; j < D; j += 64 * VEC) {
      float a[VEC], b[VEC];
      ldv<VEC>(as + base + j, a);
      ldv<VEC>(bs + base + j, b);
      stv<VEC>(a_out + base + j, a);
      stv<VEC>(b_out + base + j, b);
    }
    if constexpr (T::kAux) {
      if (c_out) {
        const float* cs = accept ? c1 : c0;
        const float* ds = accept ? d1 : d0;
        for (int64_t j = (int64_t)lane * VEC; j < D; j += 64 * VEC) {
          float a[VEC], b[VEC];
          ldv<VEC>(cs + base + j, a);
          ldv<VEC>(ds + base + j, b);
          stv<VEC>(c_out + base + j, a);
          stv<VEC>(d_out + base + j, b);
        }
      }
    }
  }
}

template <int NI, class T>
__global__ void __launch_bounds__(kBlock)
k_finish_res(Key key, int64_t off, int64_t fold, int64_t N, int64_t D, T pol, const float* __restrict__ a0,
             const float* __restrict__ logp0, const float* __restrict__ b0, const float* __restrict__ a1,
             const float* __restrict__ logp1, const float* __restrict__ b1, float* __restrict__ a_out,
             float* __restrict__ logp_out, float* __restrict__ b_out, float* __restrict__ acc_rate_out,
             uint8_t* __restrict__ is_acc_out, const float* __restrict__ aux, const float* __restrict__ c0,
             const float* __restrict__ d0, const float* __restrict__ c1, const float* __restrict__ d1,
             float* __restrict__ c_out, float* __restrict__ d_out) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = wave_row0(); r < N; r += wave_row_stride()) {
    const typename T::Row row = pol.row(r);
    const int64_t base = r * D;
    F4 A0[NI], A1[NI], B0[NI], B1[NI];
    bool ok[NI];
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      const int64_t j = ((int64_t)lane + 64 * k) * 4;
      ok[k] = j < D;
      if (ok[k]) {
        A0[k] = ld4(a0 + base + j);
        A1[k] = ld4(a1 + base + j);
        B0[k] = ld4(b0 + base + j);
        B1[k] = ld4(b1 + base + j);
      }
    }
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int k = 0; k < NI; ++k)
      if (ok[k]) {
        // aux is loaded here, not with the rows: it is not held across the select
        float ax[4] = {};
        if constexpr (T::kAux) ldv<4>(aux + ((int64_t)lane + 64 * k) * 4, ax);
        const float x0[4] = {A0[k].x, A0[k].y, A0[k].z, A0[k].w}, x1[4] = {A1[k].x, A1[k].y, A1[k].z, A1[k].w};
        const float y0[4] = {B0[k].x, B0[k].y, B0[k].z, B0[k].w}, y1[4] = {B1[k].x, B1[k].y, B1[k].z, B1[k].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) T::term(row, ax[e], x0[e], x1[e], y0[e], y1[e], s0, s1);
      }
    s0 = wave_sum(s0);
    if constexpr (T::kSums == 2) s1 = wave_sum(s1);
    const float lp0 = logp0[r], lp1 = logp1[r];
    float p_acc;
    const bool accept = metropolis_accept(key, r + off, fold, T::delta(row, s0, s1, lp0, lp1), &p_acc);
    if (lane == 0) {
      acc_rate_out[r] = p_acc;
      is_acc_out[r] = accept ? 1 : 0;
      logp_out[r] = accept ? lp1 : lp0;
    }
#pragma unroll
    for (int k = 0; k < NI; ++k)
      if (ok[k]) {
        const int64_t j = ((int64_t)lane + 64 * k) * 4;
        st4(a_out + base + j, accept ? A1[k] : A0[k]);
        st4(b_out + base + j, accept ? B1[k] : B0[k]);
      }
    if constexpr (T::kAux) {
      if (c_out) {
        const float* cs = accept ? c1 : c0;
        const float* ds = accept ? d1 : d0;
#pragma unroll
        for (int k = 0; k < NI; ++k)
          if (ok[k]) {
            const int64_t j = ((int64_t)lane + 64 * k) * 4;
            st4(c_out + base + j, ld4(cs + base + j));
            st4(d_out + base + j, ld4(ds + base + j));
          }
      }
    }
  }
}

}  // namespace bjx
