"""NumPy restatement of full-rank variational inference (TEST INFRASTRUCTURE, in the style of
meanfield_vi_restatement.py, whose optimisers it reuses).

Reference functions followed (cited by name: the reference's source is not held next to this file)
* init, step, sample, generate_fullrank_logdensity, _unflatten_cholesky      blackjax/vi/fullrank_vi.py

The approximation is ``q = N(mu, L L^T)``.  ``chol_params`` is ``(D (D + 1) / 2,)``: ``L_ii = exp(chol_params[i])`` for
``i < D``, then the strict lower triangle in ``tril_indices(D, k=-1)`` order, entry ``(i, j < i)`` at
``D + i (i - 1) / 2 + j``.  The reference's step differentiates ``kl = mean_s(logq(z_s) - logp(z_s))`` with
``z_s = mu + L eps_s`` and, under ``stl_estimator``, the parameters detached inside ``logq``.  Written out
(``G_s = grad logp(z_s)``, ``M = (1 / S) sum_s w_s eps_s^T``):

    logq_s = -|eps_s|^2 / 2 - sum_i chol_params[i] - D log(2 pi) / 2
    STL:      w_s = -u_s - G_s with L^T u_s = eps_s          not STL:  w_s = -G_s
    g_mu = mean_s w_s      g_chol[D + i (i - 1) / 2 + j] = M_ij (j < i)
    g_chol[i] = L_ii M_ii (STL)  or  -1 + L_ii M_ii (not STL)

tests/test_fullrank_vi_api.py holds these formulas against ``torch.autograd`` of the reference's literal lines.

House numerics (include/bjx_hip.h "VI").  ``eps = normal(key, (S, D))`` from the key itself; ``L_ii = exp_cr`` of the
log-diagonal (fp64 exponential rounded once to fp32); every sum is formed in fp64 from the fp32 inputs and rounded once
to fp32.  The optimiser and the additions are meanfield_vi_restatement's.
"""
from __future__ import annotations

from typing import Any, NamedTuple

import numpy as np

from meanfield_vi_restatement import LOG_2PI, SGD, Adam, AdamState  # noqa: F401  (re-exported for the tests)
from oracle import prng, targets as otargets
from oracle.fp import exp_cr, f32, f64


class FRVIState(NamedTuple):
    mu: np.ndarray
    chol_params: np.ndarray
    opt_state: Any


# ----------------------------------------------------------------------------- the packing
def num_params(D: int) -> int:
    return D * (D + 1) // 2


def index(D: int, i: int, j: int) -> int:
    """Where ``L_ij`` (``j <= i``) sits in ``chol_params``."""
    return i if i == j else D + i * (i - 1) // 2 + j


def unflatten(chol_params, diag=None) -> np.ndarray:
    """``chol_params`` -> ``L`` (D, D) in fp64.  ``diag``: the diagonal to use; by default ``exp_cr`` of the fp32
    log-diagonal (the kernels' fp32 ``L_ii``)."""
    chol = np.asarray(chol_params)
    n = chol.shape[0]
    D = (int(np.sqrt(8 * n + 1)) - 1) // 2
    assert num_params(D) == n, n
    L = np.zeros((D, D), f64)
    for i in range(D):
        L[i, :i] = chol[D + i * (i - 1) // 2: D + i * (i - 1) // 2 + i]
    L[np.arange(D), np.arange(D)] = exp_cr(chol[:D].astype(f32)) if diag is None else diag
    return L


def flatten(log_diag, L) -> np.ndarray:
    """The strict lower triangle of ``L`` behind ``log_diag``, in the packing above."""
    D = len(log_diag)
    return np.concatenate([np.asarray(log_diag)] + [np.asarray(L)[i, :i] for i in range(1, D)])


def back_substitute(L, eps) -> np.ndarray:
    """``U`` (S, D) with ``L^T u_s = eps_s``: ``u_j = (eps_j - sum_{i > j} L_ij u_i) / L_jj``, j descending."""
    L, eps = np.asarray(L), np.asarray(eps)
    D = L.shape[0]
    U = np.zeros_like(eps)
    for j in range(D - 1, -1, -1):
        U[:, j] = (eps[:, j] - U[:, j + 1:] @ L[j + 1:, j]) / L[j, j]
    return U


# ----------------------------------------------------------------------------- sample, kl_and_grad, step
def init(position, optimizer) -> FRVIState:
    mu = np.zeros_like(np.asarray(position, f32))
    chol = np.zeros(num_params(mu.shape[0]), f32)
    return FRVIState(mu, chol, optimizer.init((mu, chol)))


def noise(key, S: int, D: int) -> np.ndarray:
    return prng.normal(key, (S, D))


def sample(key, mu, chol_params, num_samples: int = 1) -> np.ndarray:
    mu, chol = np.asarray(mu, f32), np.asarray(chol_params, f32)
    eps = noise(key, num_samples, mu.shape[0]).astype(f64)
    return (mu.astype(f64)[None, :] + eps @ unflatten(chol).T).astype(f32)


def kl_and_grad_terms(eps, L, log_diag, logp, G, stl_estimator: bool = True):
    """The formulas of the module docstring on fp64 arrays: ``eps``, ``G`` (S, D), ``L`` (D, D), ``log_diag`` (D,),
    ``logp`` (S,).  -> (kl, g_mu (D,), g_chol (D (D + 1) / 2,))."""
    eps, L, log_diag, logp, G = (np.asarray(a, f64) for a in (eps, L, log_diag, logp, G))
    S, D = eps.shape
    with np.errstate(all="ignore"):
        logq = -0.5 * np.sum(eps * eps, axis=1) - np.sum(log_diag) - 0.5 * D * LOG_2PI
        kl = np.mean(logq - logp)
        w = -back_substitute(L, eps) - G if stl_estimator else -G
        g_mu = np.mean(w, axis=0)
        # M_ij = mean_s w_si eps_sj, an entry at a time: a NaN in column i of w stays in row i (a matrix product
        # through BLAS may spread it)
        M = np.stack([np.mean(w[:, i:i + 1] * eps, axis=0) for i in range(D)])
        g_diag = np.diag(L) * np.diag(M)
        if not stl_estimator:
            g_diag = -1.0 + g_diag
    return kl, g_mu, flatten(g_diag, M)


def kl_and_grad(key, mu, chol_params, logp, grad, stl_estimator: bool = True):
    """-> (kl, g_mu (D,), g_chol (D (D + 1) / 2,)) in fp64 from the fp32 inputs, the noise that of ``sample``."""
    del mu  # the gradients do not depend on it: the kernels do not read it either
    chol, G = np.asarray(chol_params, f32), np.asarray(grad, f32)
    S, D = G.shape
    return kl_and_grad_terms(noise(key, S, D), unflatten(chol), chol[:D], np.asarray(logp, f32), G, stl_estimator)


def step(key, state: FRVIState, logdensity_fn, optimizer, num_samples: int = 5, stl_estimator: bool = True):
    """``logdensity_fn``: z (S, D) fp32 -> (logp (S,), grad (S, D)) fp32.  -> (new state, kl as fp32)."""
    z = sample(key, state.mu, state.chol_params, num_samples)
    logp, G = logdensity_fn(z)
    kl, g_mu, g_chol = kl_and_grad(key, state.mu, state.chol_params, logp, G, stl_estimator)
    grads = (g_mu.astype(f32), g_chol.astype(f32))
    updates, opt_state = optimizer.update(grads, state.opt_state, (state.mu, state.chol_params))
    return FRVIState((state.mu + updates[0]).astype(f32), (state.chol_params + updates[1]).astype(f32),
                     opt_state), f32(kl)


def fullrank_logdensity(mu, cov, z) -> np.ndarray:
    """generate_fullrank_logdensity(mu, cov)(z) in fp64, closed form: -(z - mu)^T cov^-1 (z - mu) / 2
    - log det(cov) / 2 - D log(2 pi) / 2, (S,)."""
    mu, cov, z = (np.asarray(a, f64) for a in (mu, cov, z))
    d = z - mu
    _, logdet = np.linalg.slogdet(cov)
    return -0.5 * np.sum(d * np.linalg.solve(cov, d.T).T, axis=-1) - 0.5 * logdet - 0.5 * mu.shape[0] * LOG_2PI


# ----------------------------------------------------------------------------- the factors of the GPU tests
def factor_case(D: int):
    """-> (mu (D,), chol_params (D (D + 1) / 2,)) fp32 from seed ``D``: log-diagonal uniform(-1.5, 0.5), strict lower
    triangle N(0, 1) * 0.5 / sqrt(D).  test_fullrank_vi_api.py holds the condition number of every ``D`` the GPU tests
    use below 100, which keeps the back-substitution's own error far inside their tolerance."""
    rng = np.random.default_rng(D)
    log_diag = rng.uniform(-1.5, 0.5, D)
    lower = rng.standard_normal(num_params(D) - D) * 0.5 / np.sqrt(D)
    mu = rng.standard_normal(D)
    return mu.astype(f32), np.concatenate([log_diag, lower]).astype(f32)


# ----------------------------------------------------------------------------- the convergence case
CONV_RHO, CONV_D, CONV_S, CONV_STEPS, CONV_LR = 0.9, 8, 32, 600, 0.05
CONV_M = np.linspace(-2.0, 2.0, CONV_D).astype(f32)
CONV_COV = otargets.ar1_covariance(CONV_RHO, CONV_D)
CONV_SEEDS = (101, 102, 103, 104, 105)
# With STL the estimator has no variance at the optimum and a run ends at a floor of fp32 rounding noise.  Over the
# five seeds this restatement's worst was max|mu - m| = CONV_MU_WORST and max|L L^T - C| = CONV_COV_WORST; rounding
# reorders between implementations, so a run is bounded at ten times that.  Without STL the five runs ended 0.033 to
# 0.074 from m and 0.080 to 0.162 from C.
CONV_MU_WORST, CONV_COV_WORST = 9.54e-7, 1.23e-6
CONV_MU_BOUND, CONV_COV_BOUND = 10 * CONV_MU_WORST, 10 * CONV_COV_WORST


def shifted_ar1_target():
    """``oracle.targets.ar1_gaussian(0.9, 8)`` about the mean ``CONV_M``, the shift in fp32."""
    fn = otargets.ar1_gaussian(CONV_RHO, CONV_D)

    def shifted(z):
        return fn((np.asarray(z, f32) - CONV_M).astype(f32))

    return shifted


def converge(seed: int, stl_estimator: bool, steps: int = CONV_STEPS):
    """The convergence case from ``prng.key(seed)``, step ``t`` keyed ``split(key, steps)[t]``.
    -> (max|mu - m|, max|L L^T - C|, final state)."""
    opt = Adam(CONV_LR)
    fn = shifted_ar1_target()
    state = init(np.zeros(CONV_D, f32), opt)
    for k in prng.split(prng.key(seed), steps):
        state, _ = step(k, state, fn, opt, CONV_S, stl_estimator)
    return conv_errors(state.mu, state.chol_params) + (state,)


def conv_errors(mu, chol_params):
    L = unflatten(np.asarray(chol_params, f32), np.exp(np.asarray(chol_params, f64)[:CONV_D]))
    return (float(np.max(np.abs(np.asarray(mu, f64) - CONV_M.astype(f64)))),
            float(np.max(np.abs(L @ L.T - CONV_COV.astype(f64)))))


# ----------------------------------------------------------------------------- the case of the full-step tests
FULL_RHO, FULL_STEPS, FULL_LR = 0.9, 4, 0.05
# (S, D) -> seed of the four step keys, chosen so that in the restatement every coordinate of both gradients is at
# least 1e-4 in magnitude at every step (test_fullrank_vi_api.py checks it on the CPU): Adam's first update is
# -lr * g / (|g| + eps), which only a gradient next to zero makes sensitive to its last place
FULL_CASES = {(5, 3): 11, (32, 16): 11, (40, 65): 11}


def full_case(S: int, D: int):
    """-> the step keys (FULL_STEPS, 2) of the case; the target is ``oracle.targets.ar1_gaussian(FULL_RHO, D)``."""
    return prng.split(prng.key(FULL_CASES[(S, D)]), FULL_STEPS)
