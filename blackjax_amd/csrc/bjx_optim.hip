// The element-wise optimiser updates of blackjax_amd/optim.py (gfx950): optax's scale_by_adam and sgd as optim.py
// restates them, one launch per parameter.  C ABI in include/bjx_hip.h ("VI").
#include <math.h>

#include "../../include/bjx_hip.h"
#include "bjx_device.h"
#include "bjx_host.h"
#include "bjx_rows.h"

using namespace bjx;

namespace {

constexpr int64_t kMaxElems = (int64_t)1 << 31;

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

}  // namespace

extern "C" {

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
