// Mean-field variational inference (gfx950): the reparameterised draw, the reduction of an (S, D) gradient batch to
// the gradients of the variational parameters and the KL estimate, and the element-wise optimiser updates.  C ABI in
// include/bjx_hip.h ("VI").
//
// Reference: blackjax/vi/meanfield_vi.py (init, step, sample, generate_meanfield_logdensity); optax's scale_by_adam
// and sgd as blackjax_amd/optim.py restates them.
//
// A step is: the draw (one launch), the user's value-and-gradient on the (S, D) batch, the reduction (three launches:
// tiles, columns, the scalar) and one optimiser launch per parameter.  The reduction regenerates eps from the key at
// the flat index s * D + d the draw used, so no (S, D) noise array exists.  Nothing is read back, no workgroup waits on
// another, and the tiling depends on (S, D) alone: results are reproducible bit for bit.  The piece loads, stores and
// normal draws are bjx_rows.h's, the workgroup sums bjx_smc_dev.h's.
#include <math.h>

#include "../../include/bjx_hip.h"
#include "bjx_device.h"
#include "bjx_host.h"
#include "bjx_rows.h"
#include "bjx_smc_dev.h"

using namespace bjx;

namespace {

constexpr int64_t kMaxDraws = (int64_t)1 << 24;
constexpr int64_t kMaxCols = (int64_t)1 << 20;
constexpr int64_t kMaxElems = (int64_t)1 << 31;  // S * D: the partials and the flat draw index stay far inside int64
constexpr int kViTile = 64;                      // rows per workgroup of the reduction: fixed, see bjx_vi_meanfield_tile
constexpr int kKlBlock = 1024;                   // the one workgroup that forms the KL estimate
constexpr int kKlWaves = kKlBlock / BJX_WAVE;
constexpr double kHalfLog2Pi = 0.91893853320467274178;

// z[s, d] = fmaf(exp_cr(rho[d]), eps[s, d], mu[d]), eps = normal(key, (S, D)).  The rows of a batch are as few as 5
// and as long as 2^20, so the mapping is flat, not a wavefront per row: a thread owns the pieces i, i + stride, ... of
// the (S * D,) array, VEC = 4 (a piece never crosses a row: D % 4 == 0) or VEC = 1.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_vi_sample(Key key, int64_t S, int64_t D, const float* __restrict__ mu, const float* __restrict__ rho,
            float* __restrict__ z) {
  const int64_t n = S * D;
  for (int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * VEC; i < n; i += (int64_t)gridDim.x * kBlock * VEC) {
    const int64_t j = i % D;
    float m[VEC], r[VEC], e[VEC], o[VEC];
    ldv<VEC>(mu + j, m);
    ldv<VEC>(rho + j, r);
    normalv<VEC>(key, i, e);
#pragma unroll
    for (int k = 0; k < VEC; ++k) o[k] = fmaf(exp_cr(r[k]), e[k], m[k]);
    stv<VEC>(z + i, o);
  }
}

// Workgroup (tile, column block) in the column mapping of bjx_smc_dev.h (column_block, column_total), as the particle
// moments of bjx_smc.hip.  part[(tile * D + j) * 3 + {0, 1, 2}] = the tile's sums over its rows of the g_mu terms, the
// g_rho terms and eps^2 of column j, fp64.  STL: -eps / sigma - G and -eps^2 - G sigma eps; otherwise -G and
// -(G sigma eps).  Every term is formed in fp64 from the fp32 G, eps and sigma = exp_cr(rho); eps / sigma is eps times
// the fp64 reciprocal of sigma, taken once per column.
template <bool STL>
__global__ void __launch_bounds__(kBlock)
k_vi_grad_tile(Key key, int64_t S, int64_t D, int cw, const float* __restrict__ G, const float* __restrict__ rho,
               double* __restrict__ part) {
  __shared__ double sh[kBlock];
  const int tx = threadIdx.x % cw, ty = threadIdx.x / cw, groups = kBlock / cw;
  const int64_t j = (int64_t)blockIdx.y * cw + tx;
  const int64_t r0 = (int64_t)blockIdx.x * kViTile;
  const int64_t r1 = r0 + kViTile < S ? r0 + kViTile : S;
  double a_mu = 0.0, a_rho = 0.0, a_e2 = 0.0;
  if (j < D) {
    const double sig = (double)exp_cr(rho[j]);
    const double inv = 1.0 / sig;
    for (int64_t r = r0 + ty; r < r1; r += groups) {
      const int64_t i = r * D + j;
      const double e = (double)normal_from_bits(key_bits32(key, (uint64_t)i));
      const double g = (double)G[i];
      const double e2 = e * e;
      if constexpr (STL) {
        a_mu += -(e * inv) - g;
        a_rho += -e2 - g * (sig * e);
      } else {
        a_mu += -g;
        a_rho += -(g * (sig * e));
      }
      a_e2 += e2;
    }
  }
  a_mu = column_total(a_mu, sh, cw);
  a_rho = column_total(a_rho, sh, cw);
  a_e2 = column_total(a_e2, sh, cw);
  if (ty == 0 && j < D) {
    double* p = part + ((int64_t)blockIdx.x * D + j) * 3;
    p[0] = a_mu;
    p[1] = a_rho;
    p[2] = a_e2;
  }
}

// One thread per column adds the tiles in order: g_mu = sum / S and g_rho = sum / S (STL) or -1 + sum / S, rounded
// once.  colsum[2 * block + {0, 1}] = the workgroup's sums of the columns' eps^2 totals and of rho, for the KL estimate.
template <bool STL>
__global__ void __launch_bounds__(kBlock)
k_vi_grad_combine(int64_t S, int64_t D, int64_t tiles, const double* __restrict__ part, const float* __restrict__ rho,
                  float* __restrict__ g_mu, float* __restrict__ g_rho, double* __restrict__ colsum) {
  __shared__ double sh[kWavesPerBlock];
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double s_mu = 0.0, s_rho = 0.0, s_e2 = 0.0, r = 0.0;
  if (j < D) {
    for (int64_t t = 0; t < tiles; ++t) {
      const double* p = part + (t * D + j) * 3;
      s_mu += p[0];
      s_rho += p[1];
      s_e2 += p[2];
    }
    r = (double)rho[j];
    g_mu[j] = (float)(s_mu / (double)S);
    g_rho[j] = (float)(STL ? s_rho / (double)S : -1.0 + s_rho / (double)S);
  }
  s_e2 = block_sum<kWavesPerBlock>(s_e2, sh);
  r = block_sum<kWavesPerBlock>(r, sh);
  if (threadIdx.x == 0) {
    colsum[2 * blockIdx.x] = s_e2;
    colsum[2 * blockIdx.x + 1] = r;
  }
}

// kl = -(sum of eps^2) / (2 S) - sum(rho) - D log(2 pi) / 2 - mean(logp): the mean over the draws of
// logq_s - logp_s with logq_s = sum_d(-eps_sd^2 / 2 - rho_d - log(2 pi) / 2).  One workgroup, fixed order.
__global__ void __launch_bounds__(kKlBlock)
k_vi_kl(int64_t S, int64_t D, int64_t blocks, const double* __restrict__ colsum, const float* __restrict__ logp,
        float* __restrict__ kl) {
  __shared__ double sh[kKlWaves];
  double e2 = 0.0, r = 0.0, lp = 0.0;
  for (int64_t b = threadIdx.x; b < blocks; b += kKlBlock) {
    e2 += colsum[2 * b];
    r += colsum[2 * b + 1];
  }
  for (int64_t s = threadIdx.x; s < S; s += kKlBlock) lp += (double)logp[s];
  e2 = block_sum<kKlWaves>(e2, sh);
  r = block_sum<kKlWaves>(r, sh);
  lp = block_sum<kKlWaves>(lp, sh);
  if (threadIdx.x == 0)
    kl[0] = (float)(-e2 / (2.0 * (double)S) - r - (double)D * kHalfLog2Pi - lp / (double)S);
}

// optim._Adam.update, operation by operation in fp32 (no contraction: the file is built with -ffp-contract=off; the
// divisions and the square root are IEEE).  c1 = 1 - b1^count and c2 = 1 - b2^count come from the host.
__global__ void __launch_bounds__(kBlock)
k_optim_adam(int64_t n, float b1, float b2, float one_minus_b1, float one_minus_b2, float c1, float c2, float eps,
             float eps_root, float neg_lr, const float* __restrict__ g, const float* __restrict__ mu,
             const float* __restrict__ nu, float* __restrict__ mu_out, float* __restrict__ nu_out,
             float* __restrict__ u_out) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const float gi = g[i];
    const float m = (one_minus_b1 * gi) + (b1 * mu[i]);
    const float v = (one_minus_b2 * (gi * gi)) + (b2 * nu[i]);
    const float m_hat = m / c1;
    const float v_hat = v / c2;
    const float u = m_hat / (sqrtf(v_hat + eps_root) + eps);
    mu_out[i] = m;
    nu_out[i] = v;
    u_out[i] = neg_lr * u;
  }
}

// optim._SGD.update
__global__ void __launch_bounds__(kBlock)
k_optim_sgd(int64_t n, float neg_lr, const float* __restrict__ g, float* __restrict__ u_out) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    u_out[i] = neg_lr * g[i];
}

bool vi_sizes_ok(int64_t S, int64_t D) {
  return S >= 1 && S <= kMaxDraws && D >= 1 && D <= kMaxCols && S * D <= kMaxElems;
}
int64_t vi_tiles(int64_t S) { return (S + kViTile - 1) / kViTile; }
int64_t vi_col_blocks(int64_t D) { return (D + kBlock - 1) / kBlock; }

}  // namespace

extern "C" {

int bjx_vi_meanfield_tile(void) { return kViTile; }

int bjx_vi_meanfield_sample(void* stream, uint32_t key0, uint32_t key1, int64_t S, int64_t D, const float* mu,
                            const float* rho, float* z_out) {
  BJX_CHECK_ARG(vi_sizes_ok(S, D), "bjx_vi_meanfield_sample: bad sizes");
  BJX_CHECK_ARG(mu && rho && z_out, "bjx_vi_meanfield_sample: null pointer");
  const Key key{key0, key1};
  const hipStream_t s = (hipStream_t)stream;
  if (bjx_vec4_ok(D, mu, rho, z_out))
    hipLaunchKernelGGL(k_vi_sample<4>, dim3(bjx_flat_grid(S * D / 4, kBlock)), dim3(kBlock), 0, s, key, S, D, mu, rho,
                       z_out);
  else
    hipLaunchKernelGGL(k_vi_sample<1>, dim3(bjx_flat_grid(S * D, kBlock)), dim3(kBlock), 0, s, key, S, D, mu, rho,
                       z_out);
  return bjx_check_launch("bjx_vi_meanfield_sample");
}

int64_t bjx_vi_meanfield_grad_workspace_bytes(int64_t S, int64_t D) {
  if (!vi_sizes_ok(S, D)) return 0;
  // the tiles' three partials per column, then two sums per workgroup of the column launch
  return (3 * vi_tiles(S) * D + 2 * vi_col_blocks(D)) * (int64_t)sizeof(double);
}

int bjx_vi_meanfield_grad(void* stream, uint32_t key0, uint32_t key1, int64_t S, int64_t D, int32_t stl,
                          const float* G, const float* logp, const float* rho, void* workspace, float* g_mu_out,
                          float* g_rho_out, float* kl_out) {
  BJX_CHECK_ARG(vi_sizes_ok(S, D) && (stl == 0 || stl == 1), "bjx_vi_meanfield_grad: bad sizes");
  BJX_CHECK_ARG(G && logp && rho && workspace && g_mu_out && g_rho_out && kl_out,
                "bjx_vi_meanfield_grad: null pointer");
  const Key key{key0, key1};
  const hipStream_t s = (hipStream_t)stream;
  const int64_t tiles = vi_tiles(S), blocks = vi_col_blocks(D);
  const int cw = column_block(D);
  double* part = (double*)workspace;
  double* colsum = part + 3 * tiles * D;
  const dim3 tile_grid((unsigned)tiles, (unsigned)((D + cw - 1) / cw)), block(kBlock);
  if (stl) {
    hipLaunchKernelGGL(k_vi_grad_tile<true>, tile_grid, block, 0, s, key, S, D, cw, G, rho, part);
    hipLaunchKernelGGL(k_vi_grad_combine<true>, dim3((unsigned)blocks), block, 0, s, S, D, tiles, (const double*)part,
                       rho, g_mu_out, g_rho_out, colsum);
  } else {
    hipLaunchKernelGGL(k_vi_grad_tile<false>, tile_grid, block, 0, s, key, S, D, cw, G, rho, part);
    hipLaunchKernelGGL(k_vi_grad_combine<false>, dim3((unsigned)blocks), block, 0, s, S, D, tiles, (const double*)part,
                       rho, g_mu_out, g_rho_out, colsum);
  }
  hipLaunchKernelGGL(k_vi_kl, dim3(1), dim3(kKlBlock), 0, s, S, D, blocks, (const double*)colsum, logp, kl_out);
  return bjx_check_launch("bjx_vi_meanfield_grad");
}

int bjx_optim_adam(void* stream, int64_t n, float b1, float b2, float one_minus_b1, float one_minus_b2, float c1,
                   float c2, float eps, float eps_root, float neg_lr, const float* g, const float* mu, const float* nu,
                   float* mu_out, float* nu_out, float* u_out) {
  BJX_CHECK_ARG(n >= 0 && n <= kMaxElems, "bjx_optim_adam: bad sizes");
  if (n == 0) return 0;
  BJX_CHECK_ARG(g && mu && nu && mu_out && nu_out && u_out, "bjx_optim_adam: null pointer");
  hipLaunchKernelGGL(k_optim_adam, dim3(bjx_flat_grid(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, n, b1, b2,
                     one_minus_b1, one_minus_b2, c1, c2, eps, eps_root, neg_lr, g, mu, nu, mu_out, nu_out, u_out);
  return bjx_check_launch("bjx_optim_adam");
}

int bjx_optim_sgd(void* stream, int64_t n, float neg_lr, const float* g, float* u_out) {
  BJX_CHECK_ARG(n >= 0 && n <= kMaxElems, "bjx_optim_sgd: bad sizes");
  if (n == 0) return 0;
  BJX_CHECK_ARG(g && u_out, "bjx_optim_sgd: null pointer");
  hipLaunchKernelGGL(k_optim_sgd, dim3(bjx_flat_grid(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, n, neg_lr, g,
                     u_out);
  return bjx_check_launch("bjx_optim_sgd");
}

}  // extern "C"
