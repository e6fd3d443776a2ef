// Periodic orbital MCMC (gfx950).  C ABI in include/bjx_hip.h ("Periodic orbital").
//
// Reference: blackjax/mcmc/periodic_orbital.py (init, build_kernel: kernel, periodic_orbital_proposal: generate),
// jax/_src/random.py::choice, mcmc/metrics.py::gaussian_euclidean, mcmc/integrators.py::velocity_verlet.
//
// Layout and mapping: bjx_rows.h, with a chain's orbit stored as P consecutive rows: state is (N, P, D) = (N * P, D)
// row-major and one wavefront owns one CHAIN (all P rows of it), so the slot choice, the momentum draw and the softmax
// over the orbit are wave-uniform.  A transition is open -> user callable on the (N * P, D) view -> finish; per chain
// open reads 3 D floats (q, g of the chosen slot, the metric) and writes 2 P D, finish reads 2 P D + D and writes P D.
#include <math.h>

#include "../../include/bjx_hip.h"
#include "bjx_device.h"
#include "bjx_host.h"
#include "bjx_rows.h"

using namespace bjx;

namespace {

// Inclusive fp64 prefix sum over the wave's 64 lanes: the DPP sequence of wave_sum (bjx_device.h) without its final
// broadcast -- after the two row_bcast steps every lane holds the sum of lanes 0 .. itself.
__device__ __forceinline__ double wave_scan(double v) {
  v = dpp_add_f64<0x111, 0xf>(v);  // row_shr:1
  v = dpp_add_f64<0x112, 0xf>(v);  // row_shr:2
  v = dpp_add_f64<0x114, 0xf>(v);  // row_shr:4
  v = dpp_add_f64<0x118, 0xf>(v);  // row_shr:8
  v = dpp_add_f64<0x142, 0xa>(v);  // row_bcast:15 -> rows 1, 3
  v = dpp_add_f64<0x143, 0xc>(v);  // row_bcast:31 -> rows 2, 3
  return v;
}

__device__ __forceinline__ double wave_last(double v) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), 63);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), 63);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// jax/_src/random.py::choice(key_select, P, p=w): cum_j = cumsum(w)_j (each prefix accumulated in fp64, rounded once),
// r = cum_{P-1} * (1 - u) in fp32, index = searchsorted(cum, r, side="left") = #{j : cum_j < r}, at most P - 1.  The
// lanes hold 64 slots at a time; `carry` is the fp64 prefix of the chunks before.  Every lane gets the result.
__device__ __forceinline__ int64_t orbital_choice(const float* __restrict__ w, int64_t P, float u, int lane) {
  double carry = 0.0;
  for (int64_t c = 0; c < P; c += 64) {
    const int64_t j = c + lane;
    carry += wave_last(wave_scan(j < P ? (double)w[j] : 0.0));  // (lanes past P add 0: lane 63 holds the chunk's sum)
  }
  const float r = (float)carry * (1.0f - u);
  int64_t below = 0;
  carry = 0.0;
  for (int64_t c = 0; c < P; c += 64) {
    const int64_t j = c + lane;
    const double sc = wave_scan(j < P ? (double)w[j] : 0.0);
    const float cum = (float)(carry + sc);
    below += __popcll(__ballot(j < P && cum < r));
    carry += wave_last(sc);
  }
  return below < P - 1 ? below : P - 1;
}

// Opening launch.  Per chain: select the slot i ~ weights (key_select = split(chain key, 2)[1]), draw ONE momentum
// p = (1 / sqrt(imm)) * normal(key_momentum, (D,)) (key_momentum = split(chain key, 2)[0]; metrics.py gaussian_euclidean,
// the arithmetic of k_momentum_diag) and, for every slot j with its signed step s_j = float(j - d) * eps, d = directions[i],
//   drift = 1: p_half = fma(s_j / 2, g, p) ; q_j = fma(s_j, imm * p_half, q)     (velocity_verlet up to the callable)
//   drift = 0: the selected (q, p) as they are (and logp, g where asked for): the input of a user bijection.
// A row is handled in spans of 64 * VEC * NI columns whose q, g, imm and p stay in registers over the P slots; a row
// of at most one span is read once and nothing is re-read, a longer one takes one pass per span (each column is still
// drawn once: the draw is keyed by its column).
template <int VEC, int NI>
__global__ void __launch_bounds__(kBlock)
k_orbital_open(Key key, int64_t off, int64_t fold, int64_t N, int64_t P, int64_t D, int drift, float eps_s,
               const float* __restrict__ eps_pc, const float* __restrict__ imm, int64_t imm_stride,
               const float* __restrict__ weights, const int32_t* __restrict__ directions,
               const float* __restrict__ positions, const float* __restrict__ logdens,
               const float* __restrict__ grads, float* __restrict__ q_out, float* __restrict__ p_out,
               float* __restrict__ step_out, int32_t* __restrict__ choice_out, float* __restrict__ logp_rep_out,
               float* __restrict__ g_rep_out) {
  const int lane = threadIdx.x & 63;
  constexpr int64_t kSpan = 64 * VEC * NI;
  for (int64_t r = wave_row0(); r < N; r += wave_row_stride()) {
    const Key kc = chain_key(key, (uint64_t)(r + off), fold);
    const Key km = key_child(kc, 0);  // key_momentum, key_select = split(rng_key, 2)
    const float u = key_uniform(key_child(kc, 1));
    const int64_t row0 = r * P;
    const int64_t i = orbital_choice(weights + row0, P, u, lane);
    const int32_t d = directions[row0 + i];
    const float eps = eps_pc ? eps_pc[r] : eps_s;
    if (lane == 0) choice_out[r] = (int32_t)i;
    for (int64_t s = lane; s < P; s += 64) {
      step_out[row0 + s] = (float)((int32_t)s - d) * eps;
      if (logp_rep_out) logp_rep_out[row0 + s] = logdens[row0 + i];
    }
    const float* qs = positions + (row0 + i) * D;
    const float* gs = grads + (row0 + i) * D;
    const float* im = imm + r * imm_stride;
    for (int64_t c0 = 0; c0 < D; c0 += kSpan) {
      float Q[NI][VEC], G[NI][VEC], M[NI][VEC], Pm[NI][VEC];
      bool ok[NI];
#pragma unroll
      for (int k = 0; k < NI; ++k) {
        const int64_t j = c0 + ((int64_t)lane + 64 * k) * VEC;
        ok[k] = j < D;
        if (ok[k]) {
          ldv<VEC>(qs + j, Q[k]);
          ldv<VEC>(gs + j, G[k]);
          ldv<VEC>(im + j, M[k]);
          float z[VEC];
          normalv<VEC>(km, j, z);
#pragma unroll
          for (int e = 0; e < VEC; ++e) Pm[k][e] = (1.0f / sqrtf(M[k][e])) * z[e];  // two roundings, as k_momentum_diag
        }
      }
      for (int64_t s = 0; s < P; ++s) {
        const float st = (float)((int32_t)s - d) * eps;  // the reference's direction * step_size
        const float h = st * 0.5f;
        const int64_t base = (row0 + s) * D;
#pragma unroll
        for (int k = 0; k < NI; ++k)
          if (ok[k]) {
            const int64_t j = c0 + ((int64_t)lane + 64 * k) * VEC;
            float ph[VEC], qn[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
              ph[e] = drift ? fmaf(h, G[k][e], Pm[k][e]) : Pm[k][e];
              qn[e] = drift ? fmaf(st, M[k][e] * ph[e], Q[k][e]) : Q[k][e];
            }
            stv<VEC>(q_out + base + j, qn);
            stv<VEC>(p_out + base + j, ph);
            if (g_rep_out) stv<VEC>(g_rep_out + base + j, G[k]);
          }
      }
    }
  }
}

// Closing launch.  Per chain and slot j: p_j = kick ? fma(s_j / 2, g_j, p_in_j) : p_in_j (written to momentums_out),
// logw_j = logp_j - 0.5 * dot(imm * p_j, p_j) (fp64 dot rounded once, metrics.py kinetic_energy; NaN or +inf -> -inf),
// then over the chain's P slots weights = softmax(logw) (max, exp in fp64 rounded once, fp64 sum rounded once, fp32
// division), their mean and population variance (fp64, rounded once) and directions = arange(P).
// Lane l keeps the log-weights of slots l, l + 64, ...; beyond the registers they live in weights_out, which every lane
// reads back only where it wrote itself.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_orbital_finish(int64_t N, int64_t P, int64_t D, int kick, const float* __restrict__ imm, int64_t imm_stride,
                 const float* __restrict__ step, const float* __restrict__ p_in, const float* __restrict__ logp,
                 const float* __restrict__ g, float* __restrict__ mom_out, float* w_out,
                 int32_t* __restrict__ dir_out, float* __restrict__ wmean_out, float* __restrict__ wvar_out) {
  const int lane = threadIdx.x & 63;
  const float ninf = -__builtin_inff();
  for (int64_t r = wave_row0(); r < N; r += wave_row_stride()) {
    const int64_t row0 = r * P;
    const float* im = imm + r * imm_stride;
    float* w = w_out + row0;
    float m = ninf;
    for (int64_t c = 0; c < P; c += 64) {
      const int64_t cend = c + 64 < P ? c + 64 : P;
      float mine = ninf;
      for (int64_t s = c; s < cend; ++s) {
        const float h = step[row0 + s] * 0.5f;
        const int64_t base = (row0 + s) * D;
        double acc = 0.0;
        for (int64_t j = (int64_t)lane * VEC; j < D; j += 64 * VEC) {
          float pp[VEC], mm[VEC];
          ldv<VEC>(p_in + base + j, pp);
          ldv<VEC>(im + j, mm);
          if (kick) {
            float gg[VEC];
            ldv<VEC>(g + base + j, gg);
#pragma unroll
            for (int e = 0; e < VEC; ++e) pp[e] = fmaf(h, gg[e], pp[e]);
          }
          stv<VEC>(mom_out + base + j, pp);
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            const float v = mm[e] * pp[e];
            acc += (double)v * (double)pp[e];
          }
        }
        const float ke = 0.5f * (float)wave_sum(acc);
        float lw = logp[row0 + s] - ke;
        if (!(lw < __builtin_inff())) lw = ninf;  // NaN or +inf: the slot gets weight exactly 0
        if (lane == (int)(s - c)) mine = lw;
      }
      if (c + lane < P) {
        w[c + lane] = mine;
        dir_out[row0 + c + lane] = (int32_t)(c + lane);
      }
      m = fmaxf(m, mine);
    }
    m = wave_max(m);
    double sum = 0.0;
    for (int64_t j = lane; j < P; j += 64) {
      const float e = exp_cr(w[j] - m);
      w[j] = e;
      sum += (double)e;
    }
    const float S = (float)wave_sum(sum);
    sum = 0.0;
    for (int64_t j = lane; j < P; j += 64) {
      const float wj = w[j] / S;
      w[j] = wj;
      sum += (double)wj;
    }
    const double mean = wave_sum(sum) / (double)P;
    sum = 0.0;
    for (int64_t j = lane; j < P; j += 64) {
      const double dl = (double)w[j] - mean;
      sum += dl * dl;
    }
    const double var = wave_sum(sum) / (double)P;
    if (lane == 0) {
      wmean_out[r] = (float)mean;
      wvar_out[r] = (float)var;
    }
  }
}

}  // namespace

extern "C" {

int bjx_orbital_open(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold, int64_t N,
                     int64_t P, int64_t D, int drift, float eps, const float* eps_per_chain, const float* imm,
                     int64_t imm_stride, const float* weights, const int32_t* directions, const float* positions,
                     const float* logdensities, const float* grads, float* q_out, float* p_out, float* step_out,
                     int32_t* choice_out, float* logp_rep_out, float* g_rep_out) {
  BJX_CHECK_ARG(N >= 0 && D > 0 && P > 0 && P <= INT32_MAX && (imm_stride == 0 || imm_stride == D),
                "bjx_orbital_open: bad sizes");
  if (N == 0) return 0;
  BJX_CHECK_ARG(imm && weights && directions && positions && grads && q_out && p_out && step_out && choice_out &&
                    (logdensities || !logp_rep_out),
                "bjx_orbital_open: null pointer");
#define BJX_ORBITAL_OPEN(V, NI)                                                                                    \
  BJX_LAUNCH_ROWS((k_orbital_open<V, NI>), N, stream, Key{key0, key1}, chain_offset, step_fold, N, P, D, drift, eps, \
                  eps_per_chain, imm, imm_stride, weights, directions, positions, logdensities, grads, q_out, p_out, \
                  step_out, choice_out, logp_rep_out, g_rep_out)
  if (bjx_vec4_ok(D, imm, positions, grads, q_out, p_out, g_rep_out)) {
    if (D <= 256) BJX_ORBITAL_OPEN(4, 1);
    else BJX_ORBITAL_OPEN(4, 4);  // spans of 1 024 floats: resident up to there
  } else {
    BJX_ORBITAL_OPEN(1, 4);  // spans of 256 floats
  }
#undef BJX_ORBITAL_OPEN
  return bjx_check_launch("bjx_orbital_open");
}

int bjx_orbital_finish(void* stream, int64_t N, int64_t P, int64_t D, int kick, const float* imm,
                       int64_t imm_stride, const float* step, const float* p_in, const float* logp, const float* g,
                       float* momentums_out, float* weights_out, int32_t* directions_out, float* weights_mean_out,
                       float* weights_variance_out) {
  BJX_CHECK_ARG(N >= 0 && D > 0 && P > 0 && P <= INT32_MAX && (imm_stride == 0 || imm_stride == D),
                "bjx_orbital_finish: bad sizes");
  if (N == 0) return 0;
  BJX_CHECK_ARG(imm && step && p_in && logp && (g || !kick) && momentums_out && weights_out && directions_out &&
                    weights_mean_out && weights_variance_out,
                "bjx_orbital_finish: null pointer");
  BJX_LAUNCH_ROWS_VEC(bjx_vec4_ok(D, imm, p_in, g, momentums_out), k_orbital_finish, N, stream, N, P, D, kick, imm,
                      imm_stride, step, p_in, logp, g, momentums_out, weights_out, directions_out, weights_mean_out,
                      weights_variance_out);
  return bjx_check_launch("bjx_orbital_finish");
}

}  // extern "C"
