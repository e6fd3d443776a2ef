// Variational inference with a Gaussian family (gfx950): mean-field, q = N(mu, exp(rho)^2), and full-rank,
// q = N(mu, L L^T).  For each family the reparameterised draw and the reduction of an (S, D) gradient batch to the
// gradients of the variational parameters and the KL estimate.  C ABI in include/bjx_hip.h ("VI"); the optimiser
// updates of a step are bjx_optim.hip's.
//
// Reference: blackjax/vi/meanfield_vi.py and blackjax/vi/fullrank_vi.py (init, step, sample).
//
// A step is: the draw (one launch), the user's value-and-gradient on the (S, D) batch, the reduction and one optimiser
// launch per parameter.  The draw is an element-wise fma (mean-field) or a triangular product in tiles (full-rank).
// The reduction ends the same way in both families: the column sums per tile of rows, the columns, the scalar (three
// launches, one kernel pair over a family's Terms and k_vi_kl).  Full-rank has before them the blocked triangular
// solve of the sticking-the-landing term and the lower-triangular outer-product reduction.  Every kernel regenerates
// eps from the key at the flat index s * D + d the draw used, so no (S, D) noise array exists.  Nothing is read back,
// no workgroup waits on another, and the tiling depends on (S, D) alone: results are reproducible bit for bit.  The
// piece loads, stores and normal draws are bjx_rows.h's, the workgroup sums bjx_smc_dev.h's.
#include <math.h>

#include <type_traits>

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

// ----------------------------------------------------------------------------------------------------------------
// The column sums of a family: what k_vi_cols_tile adds per element and k_vi_cols_combine writes per column.  Terms
// has N, the number of fp64 sums per column, the last of them eps^2; Aux, the element type of the array beside G that
// the terms read; the per-column setup (the constructor); add, one element's terms; Out, the gradients finish writes.
//
// Mean-field: the g_mu terms, the g_rho terms and eps^2.  STL: -eps / sigma - G and -eps^2 - G sigma eps; otherwise
// -G and -(G sigma eps).  Every term is formed in fp64 from the fp32 G, eps and sigma = exp_cr(rho); eps / sigma is eps
// times the fp64 reciprocal of sigma, taken once per column.  g_mu = sum / S and g_rho = sum / S (STL) or
// -1 + sum / S, rounded once.
template <bool STL>
struct MfTerms {
  static constexpr int N = 3;
  using Aux = float;  // rho
  struct Out { float *g_mu, *g_rho; };
  double sig, inv;
  __device__ __forceinline__ MfTerms(const float* rho, int64_t j) : sig((double)exp_cr(rho[j])), inv(1.0 / sig) {}
  __device__ __forceinline__ void add(double (&a)[N], const float* G, const float*, int64_t i, double e) const {
    const double g = (double)G[i];
    const double e2 = e * e;
    if constexpr (STL) {
      a[0] += -(e * inv) - g;
      a[1] += -e2 - g * (sig * e);
    } else {
      a[0] += -g;
      a[1] += -(g * (sig * e));
    }
    a[2] += e2;
  }
  static __device__ __forceinline__ void finish(const double (&s)[N], int64_t S, int64_t j, Out out) {
    out.g_mu[j] = (float)(s[0] / (double)S);
    out.g_rho[j] = (float)(STL ? s[1] / (double)S : -1.0 + s[1] / (double)S);
  }
};

// Full-rank: w = -U - G (STL, U in W) or -G, and eps^2.  g_mu = sum / S; the outer product gives g_chol.
template <bool STL>
struct FrTerms {
  static constexpr int N = 2;
  using Aux = double;  // W
  struct Out { float* g_mu; };
  __device__ __forceinline__ FrTerms(const double*, int64_t) {}
  __device__ __forceinline__ void add(double (&a)[N], const float* G, const double* W, int64_t i, double e) const {
    a[0] += STL ? -W[i] - (double)G[i] : -(double)G[i];
    a[1] += e * e;
  }
  static __device__ __forceinline__ void finish(const double (&s)[N], int64_t S, int64_t j, Out out) {
    out.g_mu[j] = (float)(s[0] / (double)S);
  }
};

// Workgroup (tile, column block) in the column mapping of bjx_smc_dev.h (column_block, column_total), as the particle
// moments of bjx_smc.hip.  part[(tile * D + j) * N + k] = the tile's sum over its rows of term k of column j, fp64.
template <class Terms>
__global__ void __launch_bounds__(kBlock)
k_vi_cols_tile(Key key, int64_t S, int64_t D, int cw, const float* __restrict__ G,
               const typename Terms::Aux* __restrict__ aux, double* __restrict__ part) {
  constexpr int N = Terms::N;
  __shared__ double sh[kBlock];
  const int tx = threadIdx.x % cw, ty = threadIdx.x / cw, groups = kBlock / cw;
  const int64_t j = (int64_t)blockIdx.y * cw + tx;
  const int64_t r0 = (int64_t)blockIdx.x * kViTile;
  const int64_t r1 = r0 + kViTile < S ? r0 + kViTile : S;
  double a[N] = {};
  if (j < D) {
    const Terms terms(aux, j);
    for (int64_t r = r0 + ty; r < r1; r += groups) {
      const int64_t i = r * D + j;
      terms.add(a, G, aux, i, (double)normal_from_bits(key_bits32(key, (uint64_t)i)));
    }
  }
#pragma unroll
  for (int k = 0; k < N; ++k) a[k] = column_total(a[k], sh, cw);
  if (ty == 0 && j < D) {
    double* p = part + ((int64_t)blockIdx.x * D + j) * N;
#pragma unroll
    for (int k = 0; k < N; ++k) p[k] = a[k];
  }
}

// One thread per column adds the tiles in order and writes the column's gradients (Terms::finish).
// colsum[2 * block + {0, 1}] = the workgroup's sums of the columns' eps^2 totals and of the log-scale (rho, or the
// log-diagonal chol[:D]), for the KL estimate.
template <class Terms>
__global__ void __launch_bounds__(kBlock)
k_vi_cols_combine(int64_t S, int64_t D, int64_t tiles, const double* __restrict__ part,
                  const float* __restrict__ log_scale, typename Terms::Out out, double* __restrict__ colsum) {
  constexpr int N = Terms::N;
  __shared__ double sh[kWavesPerBlock];
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double s[N] = {}, r = 0.0;
  if (j < D) {
    for (int64_t t = 0; t < tiles; ++t) {
      const double* p = part + (t * D + j) * N;
#pragma unroll
      for (int k = 0; k < N; ++k) s[k] += p[k];
    }
    r = (double)log_scale[j];
    Terms::finish(s, S, j, out);
  }
  const double e2 = block_sum<kWavesPerBlock>(s[N - 1], sh);
  r = block_sum<kWavesPerBlock>(r, sh);
  if (threadIdx.x == 0) {
    colsum[2 * blockIdx.x] = e2;
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

bool vi_sizes_ok(int64_t S, int64_t D) {
  return S >= 1 && S <= kMaxDraws && D >= 1 && D <= kMaxCols && S * D <= kMaxElems;
}
int64_t vi_tiles(int64_t S) { return (S + kViTile - 1) / kViTile; }
int64_t vi_col_blocks(int64_t D) { return (D + kBlock - 1) / kBlock; }

// The three launches that end the reduction of either family.  part: Terms::N * tiles * D partials, then two sums per
// workgroup of the column launch.
template <class Terms>
void launch_cols_and_kl(hipStream_t s, Key key, int64_t S, int64_t D, const float* G, const typename Terms::Aux* aux,
                        const float* logp, const float* log_scale, double* part, typename Terms::Out out,
                        float* kl_out) {
  const int64_t tiles = vi_tiles(S), blocks = vi_col_blocks(D);
  const int cw = column_block(D);
  double* colsum = part + Terms::N * tiles * D;
  const dim3 tile_grid((unsigned)tiles, (unsigned)((D + cw - 1) / cw)), block(kBlock);
  hipLaunchKernelGGL(k_vi_cols_tile<Terms>, tile_grid, block, 0, s, key, S, D, cw, G, aux, part);
  hipLaunchKernelGGL(k_vi_cols_combine<Terms>, dim3((unsigned)blocks), block, 0, s, S, D, tiles, (const double*)part,
                     log_scale, out, colsum);
  hipLaunchKernelGGL(k_vi_kl, dim3(1), dim3(kKlBlock), 0, s, S, D, blocks, (const double*)colsum, logp, kl_out);
}

// f(std::true_type) or f(std::false_type): the launches of an estimator are written once, over a constant.
template <class F>
void with_stl(int32_t stl, F f) {
  if (stl)
    f(std::true_type{});
  else
    f(std::false_type{});
}

// ----------------------------------------------------------------------------------------------------------------
// Full-rank VI: L lower triangular and packed in chol (include/bjx_hip.h "VI"): chol[i] = log L_ii,
// L_ij = chol[D + i (i - 1) / 2 + j] for j < i, so a row of L is contiguous in j.  The triangle is cut into
// kFrBlock x kFrBlock blocks and the draws into tiles of kFrTile rows.  Every sum is an fp64 fma chain in a fixed
// order over the fp32 inputs (a product of two fp32 values is exact in fp64), rounded once to fp32 at the end.
constexpr int kFrTile = 64;    // draws per workgroup of the draw and the solve: bjx_vi_fullrank_tile
constexpr int kFrBlock = 64;   // columns per block of the triangle: bjx_vi_fullrank_block
constexpr int kFrSub = 16;     // the solve's register sub-block inside a diagonal block
constexpr int kFrOuterRows = 32;  // draws per LDS fill of the outer product
constexpr int64_t kFrMaxDraws = (int64_t)1 << 20;
constexpr int64_t kFrMaxCols = 4096;
constexpr int64_t kFrMaxElems = (int64_t)1 << 27;  // S * D: the fp64 W workspace is at most 1 GiB
constexpr int64_t kFrOuterGroups = 1024;           // the outer product splits S until about this many workgroups
constexpr int kFrMaxChunks = 64;
static_assert(kBlock == 256 && kFrTile == 64 && kFrBlock == 64, "the 16 x 16 thread grid of 4 x 4 micro-tiles");

__device__ __forceinline__ int64_t fr_row(int64_t D, int64_t i) { return D + i * (i - 1) / 2; }  // of L_i0 in chol

// eps[s + STRIDE e, j], e < 4, for the rows below `rows`: the four draws are independent straight-line code
// (normal4_from_bits), where one wavefront per SIMD would otherwise wait out four dependent chains in turn.  A row at
// or past `rows` gives 0; s >= rows gives no work at all.
template <int STRIDE>
__device__ __forceinline__ void fr_eps4(Key key, int64_t s, int64_t rows, int64_t D, int64_t j, float (&z)[4]) {
  z[0] = z[1] = z[2] = z[3] = 0.0f;
  if (s >= rows) return;
  uint32_t bits[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int64_t r = s + STRIDE * e < rows ? s + STRIDE * e : s;
    bits[e] = key_bits32(key, (uint64_t)(r * D + j));
  }
  float v[4];
  normal4_from_bits(bits, v);
#pragma unroll
  for (int e = 0; e < 4; ++e) z[e] = s + STRIDE * e < rows ? v[e] : 0.0f;
}

// A thread of a workgroup of the draw or the solve, which has the tile of ns <= kFrTile draws from s0.  As (tx, ty) of
// a 16 x 16 grid it owns the 4 x 4 fp64 micro-tile acc[a][b]: draws ty + 16 a (a < ra exist for some thread) and, of a
// block of kFrBlock columns, 4 consecutive ones (PACKED) or every 16th.  As lane `lane` of wavefront `wv` it moves the
// entries (wv + 4 e, lane), e < 16, of a block of L from memory to LDS.
struct FrTile {
  const int tx, ty, lane, wv;
  const int64_t s0;
  const int ns, ra;
  __device__ __forceinline__ explicit FrTile(int64_t S)
      : tx(threadIdx.x % 16), ty(threadIdx.x / 16), lane(threadIdx.x % 64), wv(threadIdx.x / 64),
        s0((int64_t)blockIdx.x * kFrTile), ns((int)(S - s0 < kFrTile ? S - s0 : kFrTile)), ra((ns + 15) / 16) {}
  __device__ __forceinline__ int draw(int a) const { return ty + 16 * a; }
  template <bool PACKED>
  __device__ __forceinline__ int col(int b) const { return PACKED ? 4 * tx + b : tx + 16 * b; }
};

// f(a, b) for the 16 entries of a micro-tile, unrolled.
template <class F>
__device__ __forceinline__ void fr_each(F f) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) f(a, b);
}

// f(a, b, at, in) for the entries of a micro-tile over the columns from c0 of an (S, D) array: `at` is the flat index
// of (draw, column), `in` whether both exist.
template <bool PACKED, class F>
__device__ __forceinline__ void fr_each_at(const FrTile& t, int64_t D, int64_t c0, F f) {
  fr_each([&](int a, int b) {
    const int s = t.draw(a);
    const int64_t c = c0 + t.col<PACKED>(b);
    f(a, b, (t.s0 + s) * D + c, s < t.ns && c < D);
  });
}

// The 64 x 64 block of L with rows from r0 and columns from c0 <= r0, through registers into LDS: one load per entry.
// An entry in a row past D is 0.  BELOW: the block lies below the diagonal blocks (r0 > c0).  Otherwise an entry above
// the diagonal is 0 and one on it the log-diagonal, which fr_store_L_diag then replaces.
template <bool BELOW>
__device__ __forceinline__ void fr_load_L_block(const FrTile& t, int64_t D, const float* __restrict__ chol,
                                                int64_t r0, int64_t c0, float (&l)[kFrBlock / 4]) {
  const int64_t j = c0 + t.lane;
#pragma unroll
  for (int e = 0; e < kFrBlock / 4; ++e) {
    const int64_t i = r0 + t.wv + 4 * e;
    if (BELOW)
      l[e] = i < D ? chol[fr_row(D, i) + j] : 0.0f;
    else
      l[e] = (i < D && j <= i) ? chol[j < i ? fr_row(D, i) + j : i] : 0.0f;
  }
}

template <class T, int LD>
__device__ __forceinline__ void fr_store_L_block(const FrTile& t, const float (&l)[kFrBlock / 4],
                                                 T (&Ls)[kFrBlock][LD]) {
#pragma unroll
  for (int e = 0; e < kFrBlock / 4; ++e) Ls[t.wv + 4 * e][t.lane] = (T)l[e];
}

// Of a diagonal block (r0 == c0): Ls[lane][lane] = diag(log L of that entry), by the thread that loaded row `lane` up
// to its diagonal -- one transcendental per lane.
template <class T, int LD, class F>
__device__ __forceinline__ void fr_store_L_diag(const FrTile& t, const float (&l)[kFrBlock / 4],
                                                T (&Ls)[kFrBlock][LD], F diag) {
  if (t.wv != t.lane % 4) return;
  float d = 0.0f;
#pragma unroll
  for (int e = 0; e < kFrBlock / 4; ++e) d = t.lane == t.wv + 4 * e ? l[e] : d;
  Ls[t.lane][t.lane] = diag(d);
}

// z[s, i] = fp32(mu_i + sum_{j <= i} L_ij eps_sj), j ascending.  Workgroup (tile of kFrTile draws, block I of
// kFrBlock columns) walks the column chunks 0 .. I of eps (those wholly above the diagonal are skipped), regenerates a
// chunk into LDS once and reads the rows of L contiguously.  Thread (tx, ty) owns draws ty + 16 a and columns
// tx + 16 b, a, b < 4; a tile with fewer than 64 draws skips the a it does not have.
__global__ void __launch_bounds__(kBlock)
k_fr_sample(Key key, int64_t S, int64_t D, const float* __restrict__ mu, const float* __restrict__ chol,
            float* __restrict__ z) {
  __shared__ float Ls[kFrBlock][kFrBlock + 1];
  __shared__ float eS[kFrTile][kFrBlock + 1];
  const FrTile t(S);
  const int I = blockIdx.y;
  const int64_t i0 = (int64_t)I * kFrBlock;
  double acc[4][4] = {};
  // the next chunk's entries of L are loaded while this one is used
  float lreg[kFrBlock / 4];
  fr_load_L_block<false>(t, D, chol, i0, 0, lreg);
  for (int c = 0; c <= I; ++c) {
    const int64_t j = (int64_t)c * kFrBlock + t.lane;
    __syncthreads();
    fr_store_L_block(t, lreg, Ls);
    if (c == I && i0 + t.lane < D) fr_store_L_diag(t, lreg, Ls, [](float d) { return exp_cr(d); });
    for (int e4 = 0; e4 < kFrTile / 16; ++e4) {
      float ev[4];
      fr_eps4<4>(key, t.s0 + t.wv + 16 * e4, j < D ? t.s0 + t.ns : 0, D, j, ev);
#pragma unroll
      for (int e = 0; e < 4; ++e) eS[t.wv + 16 * e4 + 4 * e][t.lane] = ev[e];
    }
    __syncthreads();
    if (c < I) fr_load_L_block<false>(t, D, chol, i0, (int64_t)(c + 1) * kFrBlock, lreg);
    for (int jj = 0; jj < kFrBlock; ++jj) {
      double l[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) l[b] = (double)Ls[t.col<false>(b)][jj];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        if (a < t.ra) {
          const double ev = (double)eS[t.draw(a)][jj];
#pragma unroll
          for (int b = 0; b < 4; ++b) acc[a][b] = fma(l[b], ev, acc[a][b]);
        }
      }
    }
  }
  fr_each_at<false>(t, D, i0, [&](int a, int b, int64_t at, bool in) {
    if (in) z[at] = (float)((double)mu[i0 + t.col<false>(b)] + acc[a][b]);
  });
}

// STL only: L^T u_s = eps_s, U in fp64 into W, by a right-looking blocked back-substitution from the last column
// block to the first, one launch per column block: the launch-separated form of a loop that a single workgroup per
// tile of draws ran 10 to 20 times slower.  The running right-hand side r lives in W (columns not yet
// solved) and starts as eps, regenerated where it is first needed.  Launch t = nb - 1 .. 0, workgroup (tile of
// kFrTile draws, block K <= t): r_K -= sum_i L_iK u_i over the rows i of block t + 1, i descending (the block the
// launch before solved; nothing for t = nb - 1, which has one workgroup per tile); then K < t writes r_K back, and K = t
// solves its diagonal block -- L's block with its diagonal replaced by the fp64 reciprocals of L_jj and r to LDS, one
// wavefront (a lane per draw) in register sub-blocks of kFrSub columns, u_j = r_j (1 / L_jj), then r_i -= L_ji u_j
// for i < j, j descending -- and writes u.  Thread (tx, ty) owns draws ty + 16 a and columns 4 tx + b of its block.
__global__ void __launch_bounds__(kBlock)
k_fr_solve_step(Key key, int64_t S, int64_t D, int t, const float* __restrict__ chol, double* W) {
  __shared__ double Ls[kFrBlock][kFrBlock];  // [row of L][column of L]
  __shared__ double rT[kFrBlock][kFrTile];   // [column][draw]: u of block t + 1, then r and u of block t
  const FrTile th(S);
  const int lane = th.lane, wv = th.wv;
  const int nb = (int)((D + kFrBlock - 1) / kFrBlock);
  const bool upd = t + 1 < nb;
  const bool fresh = t + 2 >= nb;  // no launch has written r yet: it is eps
  const int K = upd ? (int)blockIdx.y : t;
  const int64_t k0 = (int64_t)K * kFrBlock;
  double acc[4][4];
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int64_t k = k0 + th.col<true>(b);
    float ev[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (fresh) fr_eps4<16>(key, th.s0 + th.ty, k < D ? th.s0 + th.ns : 0, D, k, ev);
#pragma unroll
    for (int a = 0; a < 4; ++a) acc[a][b] = (double)ev[a];
  }
  if (!fresh)
    fr_each_at<true>(th, D, k0, [&](int a, int b, int64_t at, bool in) {
      if (in) acc[a][b] = W[at];
    });
  float l[kFrBlock / 4];
  if (upd) {
    const int64_t j0 = (int64_t)(t + 1) * kFrBlock;
    fr_load_L_block<true>(th, D, chol, j0, k0, l);
    fr_each_at<true>(th, D, j0, [&](int a, int b, int64_t at, bool in) {
      rT[th.col<true>(b)][th.draw(a)] = in ? W[at] : 0.0;
    });
    fr_store_L_block(th, l, Ls);
    __syncthreads();
    for (int ii = kFrBlock - 1; ii >= 0; --ii) {
      double lv[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) lv[b] = Ls[ii][th.col<true>(b)];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        if (a < th.ra) {
          const double u = rT[ii][th.draw(a)];
#pragma unroll
          for (int b = 0; b < 4; ++b) acc[a][b] = fma(-lv[b], u, acc[a][b]);
        }
      }
    }
    if (K < t) {  // a block left of the last: all its columns exist, and pairs of them go out in one store
      fr_each_at<true>(th, D, k0, [&](int a, int b, int64_t at, bool) {
        if (th.draw(a) < th.ns) W[at] = acc[a][b];
      });
      return;
    }
    __syncthreads();
  }
  // K == t: the diagonal block
  fr_load_L_block<false>(th, D, chol, k0, k0, l);
  fr_store_L_block(th, l, Ls);
  fr_store_L_diag(th, l, Ls, [&](float d) { return k0 + lane < D ? 1.0 / (double)exp_cr(d) : 1.0; });
  fr_each([&](int a, int b) { rT[th.col<true>(b)][th.draw(a)] = acc[a][b]; });
  __syncthreads();
  // a lane per draw; the triangle of a sub-block is one wavefront's, the columns to its left are shared by the four
  for (int c = kFrBlock / kFrSub - 1; c >= 0; --c) {
    const int c0 = c * kFrSub;
    double r[kFrSub];
    if (wv == 0) {
#pragma unroll
      for (int q = 0; q < kFrSub; ++q) r[q] = rT[c0 + q][lane];
#pragma unroll
      for (int q = kFrSub - 1; q >= 0; --q) {
        r[q] = r[q] * Ls[c0 + q][c0 + q];
#pragma unroll
        for (int p = 0; p < q; ++p) r[p] = fma(-Ls[c0 + q][c0 + p], r[q], r[p]);
      }
#pragma unroll
      for (int q = 0; q < kFrSub; ++q) rT[c0 + q][lane] = r[q];
    }
    __syncthreads();
    if (c == 0) break;
#pragma unroll
    for (int q = 0; q < kFrSub; ++q) r[q] = rT[c0 + q][lane];
#pragma unroll 4
    for (int i = wv; i < c0; i += 4) {
      double v = rT[i][lane];
#pragma unroll
      for (int q = kFrSub - 1; q >= 0; --q) v = fma(-Ls[c0 + q][i], r[q], v);
      rT[i][lane] = v;
    }
    __syncthreads();
  }
  fr_each_at<true>(th, D, k0, [&](int a, int b, int64_t at, bool in) {
    if (in) W[at] = rT[th.col<true>(b)][th.draw(a)];
  });
}

// Block p of the lower triangle, row-major over (I, J <= I).
__device__ __forceinline__ void fr_block_of(int p, int* I, int* J) {
  int i = 0;
  while ((i + 1) * (i + 2) / 2 <= p) ++i;
  *I = i;
  *J = p - i * (i + 1) / 2;
}

// part[((chunk * nbt + p) * 64 + ii) * 64 + jj] = sum over the chunk's draws, in order, of w_s[I 64 + ii] eps_s[J 64 + jj]
// with w = -U - G (STL, U in W) or -G.  Workgroup (block p = (I, J) of the triangle, chunk of `rows` draws); the eps columns of J
// are regenerated.  Thread (tx, ty) owns rows 4 ty + a and columns 4 tx + b of the block.
template <bool STL>
__global__ void __launch_bounds__(kBlock)
k_fr_outer(Key key, int64_t S, int64_t D, int64_t rows, int nbt, const float* __restrict__ G,
           const double* __restrict__ W, double* __restrict__ part) {
  __shared__ double wS[kFrOuterRows][kFrBlock];
  __shared__ double eS[kFrOuterRows][kFrBlock];
  const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16, lane = tid % 64, wv = tid / 64;
  int I, J;
  fr_block_of((int)blockIdx.x, &I, &J);
  const int64_t i = (int64_t)I * kFrBlock + lane, j = (int64_t)J * kFrBlock + lane;
  const int64_t sbeg = (int64_t)blockIdx.y * rows;
  const int64_t send = sbeg + rows < S ? sbeg + rows : S;
  double acc[4][4] = {};
  for (int64_t st = sbeg; st < send; st += kFrOuterRows) {
    __syncthreads();
    for (int e = 0; e < kFrOuterRows / 4; ++e) {
      const int r = wv + 4 * e;
      const int64_t s = st + r;
      double w = 0.0;
      if (s < send && i < D) w = STL ? -W[s * D + i] - (double)G[s * D + i] : -(double)G[s * D + i];
      wS[r][lane] = w;
    }
    for (int e4 = 0; e4 < kFrOuterRows / 16; ++e4) {
      float ev[4];
      fr_eps4<4>(key, st + wv + 16 * e4, j < D ? send : 0, D, j, ev);
#pragma unroll
      for (int e = 0; e < 4; ++e) eS[wv + 16 * e4 + 4 * e][lane] = (double)ev[e];
    }
    __syncthreads();
    for (int r = 0; r < kFrOuterRows; ++r) {
      double w[4], ev[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) w[a] = wS[r][4 * ty + a];
#pragma unroll
      for (int b = 0; b < 4; ++b) ev[b] = eS[r][4 * tx + b];
      fr_each([&](int a, int b) { acc[a][b] = fma(w[a], ev[b], acc[a][b]); });
    }
  }
  double* out = part + ((int64_t)blockIdx.y * nbt + blockIdx.x) * (kFrBlock * kFrBlock);
  fr_each([&](int a, int b) { out[(4 * ty + a) * kFrBlock + 4 * tx + b] = acc[a][b]; });
}

// One thread per entry of a block adds the chunks in order: M_ij = sum / S, the packed entry for j < i and, on the
// diagonal, g_chol[i] = L_ii M_ii (STL) or -1 + L_ii M_ii, rounded once.
template <bool STL>
__global__ void __launch_bounds__(kBlock)
k_fr_outer_combine(int64_t S, int64_t D, int chunks, int nbt, const double* __restrict__ part,
                   const float* __restrict__ chol, float* __restrict__ g_chol) {
  constexpr int kPerGroup = kFrBlock * kFrBlock / kBlock;  // workgroups per block of the triangle
  const int p = blockIdx.x / kPerGroup;
  const int e = (blockIdx.x % kPerGroup) * kBlock + threadIdx.x;
  int I, J;
  fr_block_of(p, &I, &J);
  const int64_t i = (int64_t)I * kFrBlock + e / kFrBlock, j = (int64_t)J * kFrBlock + e % kFrBlock;
  if (i >= D || j > i) return;
  double m = 0.0;
  for (int c = 0; c < chunks; ++c) m += part[((int64_t)c * nbt + p) * (kFrBlock * kFrBlock) + e];
  m /= (double)S;
  if (j < i) {
    g_chol[fr_row(D, i) + j] = (float)m;
  } else {
    const double lm = (double)exp_cr(chol[i]) * m;
    g_chol[i] = (float)(STL ? lm : -1.0 + lm);
  }
}

bool fr_sizes_ok(int64_t S, int64_t D) {
  return S >= 1 && S <= kFrMaxDraws && D >= 1 && D <= kFrMaxCols && S * D <= kFrMaxElems;
}
int64_t fr_tiles(int64_t S) { return (S + kFrTile - 1) / kFrTile; }
int64_t fr_blocks(int64_t D) { return (D + kFrBlock - 1) / kFrBlock; }
int64_t fr_tri_blocks(int64_t D) { return fr_blocks(D) * (fr_blocks(D) + 1) / 2; }
// Draws per chunk of the outer product, a multiple of its LDS fill: S is split until the launch has about
// kFrOuterGroups workgroups, into at most kFrMaxChunks chunks.  A function of (S, D) alone.
int64_t fr_chunk_rows(int64_t S, int64_t D) {
  const int64_t fills = (S + kFrOuterRows - 1) / kFrOuterRows;
  int64_t want = kFrOuterGroups / fr_tri_blocks(D);
  want = want < 1 ? 1 : (want > kFrMaxChunks ? kFrMaxChunks : want);
  const int64_t chunks = want < fills ? want : fills;
  return (fills + chunks - 1) / chunks * kFrOuterRows;
}
int64_t fr_chunks(int64_t S, int64_t D) {
  const int64_t rows = fr_chunk_rows(S, D);
  return (S + rows - 1) / rows;
}

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
  with_stl(stl, [&](auto c) {
    launch_cols_and_kl<MfTerms<decltype(c)::value>>((hipStream_t)stream, Key{key0, key1}, S, D, G, rho, logp, rho,
                                                    (double*)workspace, {g_mu_out, g_rho_out}, kl_out);
  });
  return bjx_check_launch("bjx_vi_meanfield_grad");
}

int bjx_vi_fullrank_tile(void) { return kFrTile; }
int bjx_vi_fullrank_block(void) { return kFrBlock; }

int bjx_vi_fullrank_sample(void* stream, uint32_t key0, uint32_t key1, int64_t S, int64_t D, const float* mu,
                           const float* chol, float* z_out) {
  BJX_CHECK_ARG(fr_sizes_ok(S, D), "bjx_vi_fullrank_sample: bad sizes");
  BJX_CHECK_ARG(mu && chol && z_out, "bjx_vi_fullrank_sample: null pointer");
  const dim3 grid((unsigned)fr_tiles(S), (unsigned)fr_blocks(D));
  hipLaunchKernelGGL(k_fr_sample, grid, dim3(kBlock), 0, (hipStream_t)stream, Key{key0, key1}, S, D, mu, chol, z_out);
  return bjx_check_launch("bjx_vi_fullrank_sample");
}

int64_t bjx_vi_fullrank_grad_workspace_bytes(int64_t S, int64_t D) {
  if (!fr_sizes_ok(S, D)) return 0;
  // W, the outer product's partial blocks, the tiles' two partials per column, two sums per workgroup of the columns
  return (S * D + fr_chunks(S, D) * fr_tri_blocks(D) * kFrBlock * kFrBlock + 2 * vi_tiles(S) * D +
          2 * vi_col_blocks(D)) * (int64_t)sizeof(double);
}

int bjx_vi_fullrank_grad(void* stream, uint32_t key0, uint32_t key1, int64_t S, int64_t D, int32_t stl,
                         const float* G, const float* logp, const float* chol, void* workspace, float* g_mu_out,
                         float* g_chol_out, float* kl_out) {
  BJX_CHECK_ARG(fr_sizes_ok(S, D) && (stl == 0 || stl == 1), "bjx_vi_fullrank_grad: bad sizes");
  BJX_CHECK_ARG(G && logp && chol && workspace && g_mu_out && g_chol_out && kl_out,
                "bjx_vi_fullrank_grad: null pointer");
  const Key key{key0, key1};
  const hipStream_t s = (hipStream_t)stream;
  const int64_t rows = fr_chunk_rows(S, D);
  const int chunks = (int)fr_chunks(S, D), nbt = (int)fr_tri_blocks(D), nb = (int)fr_blocks(D);
  double* W = (double*)workspace;
  double* outer = W + S * D;
  double* part = outer + (int64_t)chunks * nbt * kFrBlock * kFrBlock;
  const dim3 block(kBlock), outer_grid((unsigned)nbt, (unsigned)chunks);
  const dim3 combine_grid((unsigned)(nbt * (kFrBlock * kFrBlock / kBlock)));
  with_stl(stl, [&](auto c) {
    constexpr bool STL = decltype(c)::value;
    if constexpr (STL)
      for (int t = nb - 1; t >= 0; --t)
        hipLaunchKernelGGL(k_fr_solve_step, dim3((unsigned)fr_tiles(S), (unsigned)(t + 1 < nb ? t + 1 : 1)), block, 0,
                           s, key, S, D, t, chol, W);
    hipLaunchKernelGGL(k_fr_outer<STL>, outer_grid, block, 0, s, key, S, D, rows, nbt, G, (const double*)W, outer);
    hipLaunchKernelGGL(k_fr_outer_combine<STL>, combine_grid, block, 0, s, S, D, chunks, nbt, (const double*)outer,
                       chol, g_chol_out);
    launch_cols_and_kl<FrTerms<STL>>(s, key, S, D, G, (const double*)W, logp, chol, part, {g_mu_out}, kl_out);
  });
  return bjx_check_launch("bjx_vi_fullrank_grad");
}

}  // extern "C"
