"""NumPy restatement of the marginal latent-Gaussian transition (TEST INFRASTRUCTURE, in the style of
tests/mala_restatement.py).

Batched with a leading chain axis; chain ``i`` of ``kernel(rng_key, state, ...)`` follows the reference's single-chain
``blackjax.mgrad_gaussian.build_kernel(cov_svd)(jax.random.split(rng_key, N)[chain_offset + i], state_i, ...)``.

Reference functions followed (cited by name: the reference's source is not held next to this file)
* MarginalState / MarginalInfo / CovarianceSVD / init   blackjax/mcmc/marginal_latent_gaussian.py
* build_kernel (kernel), generate_mean_shifted_logprob   blackjax/mcmc/marginal_latent_gaussian.py
* static_binomial_sampling, safe_energy_diff             blackjax/mcmc/proposal.py

The model is a prior ``N(0, C)``, ``C = U diag(Gamma) U_t``, times ``exp(logdensity_fn)``.  ``cov_svd`` is taken as fp32
arrays ``(U, Gamma, U_t)`` -- the factorisation is never part of a comparison -- and ``U is None`` is a diagonal prior
(``U = I``, no product).  One transition of one chain, with ``y_key, u_key = split(chain key, 2)``:

    Gamma_1 = Gamma delta / (delta + 2 Gamma) ; Gamma_3 = (delta + 2 Gamma) / (delta + 4 Gamma) ; Gamma_2 = Gamma_1 / Gamma_3
    t = Gamma_1 (U_x / (0.5 delta) + U_grad_x) + sqrt(Gamma_2) normal(y_key, (D,)) ; y = U t
    U_y = U_t y ; U_grad_y = U_t grad(y)
    t_x = Gamma_1 (U_x / (0.5 delta) + 0.5 U_grad_x) ; t_y likewise
    hxy = dot(U_x - t_y, Gamma_3 U_grad_y) ; hyx = dot(U_y - t_x, Gamma_3 U_grad_x)
    log_ratio = logp_y - logp_x + hxy - hyx ; accept = uniform(u_key) < min(1, exp(log_ratio))

House numerics: fp32 as written, left to right; every ``x + s * y`` one fused multiply-add;
divisions and sqrt correctly rounded; the two dots over D in fp64 rounded once; exp in fp64 rounded once;
``log_ratio = ((logp_y - logp_x) + hxy) - hyx``; a NaN log_ratio rejects with acceptance rate 0 (safe_energy_diff);
the three products with ``U`` / ``U_t`` are the engine's fp32 fma chains in the MFMA k order.  ``transition_f64`` is
the same transition in plain fp64 without house rounding.  Parity of the random streams with a real JAX run is
unpinned, as for the rest of the RNG-dependent surface.
"""
from __future__ import annotations

from typing import Callable, NamedTuple

import numpy as np

from oracle import cport, prng
from oracle.fp import dot64, exp_cr, f32, fma32, gemm_f32chain, mfma_k_order, sqrt32
from oracle.hmc import safe_energy_diff

f64 = np.float64


class MarginalState(NamedTuple):
    position: np.ndarray  # (N, D)
    logdensity: np.ndarray  # (N,)
    logdensity_grad: np.ndarray  # (N, D)
    U_x: np.ndarray  # (N, D)
    U_grad_x: np.ndarray  # (N, D)


class MarginalInfo(NamedTuple):
    acceptance_rate: np.ndarray  # (N,) float32
    is_accepted: np.ndarray  # (N,) bool
    proposal: MarginalState


class CovarianceSVD(NamedTuple):
    U: np.ndarray | None  # (D, D) float32, or None: diagonal prior
    Gamma: np.ndarray  # (D,) float32
    U_t: np.ndarray | None


def matmul(a, b_kn):
    """``a @ b_kn`` as the engine's GEMMs evaluate it: one fp32 fma chain per element in the MFMA k order.  The C port
    serves large shapes (bit-identical to oracle.fp.gemm_f32chain, tests/test_oracle_c.py)."""
    a = np.ascontiguousarray(a, dtype=f32)
    b_kn = np.ascontiguousarray(b_kn, dtype=f32)
    order = mfma_k_order(a.shape[1])
    if a.shape[0] * a.shape[1] * b_kn.shape[1] > (1 << 22):
        return cport.gemm_f32chain(a, b_kn, order)
    return gemm_f32chain(a, b_kn, order)


def mean_shifted(logdensity_fn: Callable, shift) -> Callable:
    """generate_mean_shifted_logprob with its gradient: (logp + dot(x, shift), g + shift), ``shift = C^-1 mean``."""
    shift = np.asarray(shift, f32)

    def fn(x):
        logp, g = logdensity_fn(x)
        with np.errstate(invalid="ignore", over="ignore"):
            return (np.asarray(logp, f32) + dot64(x, shift)).astype(f32), (np.asarray(g, f32) + shift).astype(f32)

    return fn


def shift_from_svd(cov_svd: CovarianceSVD, mean) -> np.ndarray:
    """``U ((U_t mean) / Gamma)`` from the fp32 factor in fp64, rounded once (what the engine does on the host)."""
    U, gamma, U_t = cov_svd
    m = np.broadcast_to(np.asarray(mean, f64), gamma.shape)
    if U is None:
        return (m / gamma.astype(f64)).astype(f32)
    return (U.astype(f64) @ ((U_t.astype(f64) @ m) / gamma.astype(f64))).astype(f32)


def init(position, logdensity_fn: Callable, cov_svd: CovarianceSVD) -> MarginalState:
    position = np.asarray(position, dtype=f32)
    with np.errstate(all="ignore"):
        logp, grad = logdensity_fn(position)
    logp, grad = np.asarray(logp, f32), np.asarray(grad, f32)
    if cov_svd.U is None:
        return MarginalState(position, logp, grad, position, grad)
    return MarginalState(position, logp, grad, matmul(position, cov_svd.U), matmul(grad, cov_svd.U))


def _coef(gamma, delta_col):
    d2 = fma32(f32(2.0), gamma, delta_col)  # delta + 2 Gamma (the product is exact)
    d4 = fma32(f32(4.0), gamma, delta_col)
    g1 = ((gamma * delta_col).astype(f32) / d2).astype(f32)
    g3 = (d2 / d4).astype(f32)
    return g1, g3


def kernel(rng_key, state: MarginalState, logdensity_fn, cov_svd: CovarianceSVD, delta, chain_offset: int = 0,
           chain_keys_override=None):
    """One transition of every chain.  ``delta``: a scalar or (N,).  ``chain_keys_override``: (N, 2) per-chain keys used
    instead of ``split(rng_key, .)[chain_offset : chain_offset + N]`` (the chain-major key layout)."""
    x, logp_x, g_x, U_x, U_grad_x = state
    U, gamma, U_t = cov_svd
    gamma = np.asarray(gamma, f32)
    N, D = x.shape
    delta_col = np.broadcast_to(np.asarray(delta, dtype=f32), (N,)).astype(f32)[:, None]
    hd = (f32(0.5) * delta_col).astype(f32)
    keys = prng.split(rng_key, N, offset=chain_offset) if chain_keys_override is None else chain_keys_override
    kk = prng.split(keys, 2)  # y_key, u_key
    z = prng.normal(kk[:, 0], (D,))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        g1, g3 = _coef(gamma, delta_col)
        s = sqrt32((g1 / g3).astype(f32))  # sqrt(Gamma_2)
        t = fma32(s, z, (g1 * ((U_x / hd).astype(f32) + U_grad_x).astype(f32)).astype(f32))
        y = t if U is None else matmul(t, U_t)
    with np.errstate(all="ignore"):
        logp_y, g_y = logdensity_fn(y)
    logp_y, g_y = np.asarray(logp_y, f32), np.asarray(g_y, f32)
    if U is None:
        U_y, U_grad_y = y, g_y
    else:
        with np.errstate(invalid="ignore", over="ignore"):
            U_y, U_grad_y = matmul(y, U), matmul(g_y, U)
    with np.errstate(invalid="ignore", over="ignore"):
        t_x = (g1 * fma32(f32(0.5), U_grad_x, (U_x / hd).astype(f32))).astype(f32)
        t_y = (g1 * fma32(f32(0.5), U_grad_y, (U_y / hd).astype(f32))).astype(f32)
        hxy = dot64((U_x - t_y).astype(f32), (g3 * U_grad_y).astype(f32))
        hyx = dot64((U_y - t_x).astype(f32), (g3 * U_grad_x).astype(f32))
        log_ratio = (((logp_y - logp_x).astype(f32) + hxy).astype(f32) - hyx).astype(f32)
    d = safe_energy_diff(log_ratio, f32(0.0))
    p_acc = np.minimum(exp_cr(d), f32(1.0))
    acc = prng.uniform(kk[:, 1], ()) < p_acc  # static_binomial_sampling
    am = acc[:, None]
    proposal = MarginalState(y, logp_y, g_y, U_y, U_grad_y)
    new_state = MarginalState(np.where(am, y, x).astype(f32), np.where(acc, logp_y, logp_x).astype(f32),
                              np.where(am, g_y, g_x).astype(f32), np.where(am, U_y, U_x).astype(f32),
                              np.where(am, U_grad_y, U_grad_x).astype(f32))
    if U is None:  # the eigenbasis images ARE the position and the gradient
        new_state = new_state._replace(U_x=new_state.position, U_grad_x=new_state.logdensity_grad)
    return new_state, MarginalInfo(p_acc.astype(f32), acc, proposal)


# ---- the same transition in plain fp64, without house rounding ---------------------------------------------------


def proposal_moments_f64(x, g_x, U, gamma, delta):
    """Mean and (diagonal) variance, in the eigenbasis, of ``q(. | x)``: ``U_t y ~ N(mean, diag(var))``."""
    g1 = gamma * delta / (delta + 2.0 * gamma)
    g3 = (delta + 2.0 * gamma) / (delta + 4.0 * gamma)
    return g1 * ((x @ U) / (0.5 * delta) + g_x @ U), g1 / g3


def log_ratio_f64(x, logp_x, g_x, y, logp_y, g_y, U, gamma, delta):
    """The log acceptance ratio of the transition formulas, fp64, (N,) for (N, D) rows.  ``U`` is (D, D)."""
    g1 = gamma * delta / (delta + 2.0 * gamma)
    g3 = (delta + 2.0 * gamma) / (delta + 4.0 * gamma)
    U_x, U_gx, U_y, U_gy = x @ U, g_x @ U, y @ U, g_y @ U
    t_x = g1 * (U_x / (0.5 * delta) + 0.5 * U_gx)
    t_y = g1 * (U_y / (0.5 * delta) + 0.5 * U_gy)
    hxy = np.sum((U_x - t_y) * (g3 * U_gy), -1)
    hyx = np.sum((U_y - t_x) * (g3 * U_gx), -1)
    return logp_y - logp_x + hxy - hyx


def transition_f64(rng: np.random.Generator, x, logp_x, g_x, logdensity_fn, U, gamma, delta):
    """One transition of every row in fp64 with NumPy's generator; returns (x, logp, g, acceptance probability)."""
    mean, var = proposal_moments_f64(x, g_x, U, gamma, delta)
    y = (mean + np.sqrt(var) * rng.standard_normal(x.shape)) @ U.T
    logp_y, g_y = logdensity_fn(y)
    alpha = np.exp(np.minimum(0.0, log_ratio_f64(x, logp_x, g_x, y, logp_y, g_y, U, gamma, delta)))
    acc = rng.random(x.shape[0]) < alpha
    am = acc[:, None]
    return np.where(am, y, x), np.where(acc, logp_y, logp_x), np.where(am, g_y, g_x), alpha


# ---- the Gaussian-likelihood case with a closed-form posterior (stationarity checks) ------------------------------


class StationarityCase(NamedTuple):
    cov_svd: CovarianceSVD  # fp32 factor of the prior covariance
    mean: np.ndarray  # (D,) float32 prior mean
    inv_var: np.ndarray  # (D,) float32: the likelihood is oracle.targets.diag_gaussian(inv_var)
    x0: np.ndarray  # (N, D) float32 start
    post_mean: np.ndarray  # (D,) float64
    post_var: np.ndarray  # (D,) float64 marginal variances
    n_steps: int


def random_factor(D: int, seed: int = 5) -> CovarianceSVD:
    """U from the QR of an oracle.prng normal matrix rounded to fp32, U_t its exact transpose,
    Gamma = 10^linspace(-1, 1, D)."""
    q, _ = np.linalg.qr(prng.normal(prng.key(seed), (D, D)).astype(f64))
    U = np.ascontiguousarray(q.astype(f32))
    return CovarianceSVD(U, (10.0 ** np.linspace(-1.0, 1.0, D)).astype(f32), np.ascontiguousarray(U.T))


def stationarity_case(D: int = 16, N: int = 512, n_steps: int = 200) -> StationarityCase:
    """Prior N(mean, U diag(Gamma) U_t), likelihood exp(-0.5 sum inv_var x^2): the posterior is Gaussian with precision
    P = C^-1 + diag(inv_var) and mean P^-1 C^-1 mean."""
    svd = random_factor(D)
    mean = np.linspace(-1.0, 2.0, D).astype(f32)
    inv_var = (10.0 ** np.linspace(0.5, -0.5, D)).astype(f32)
    U, gamma = svd.U.astype(f64), svd.Gamma.astype(f64)
    prec = U @ np.diag(1.0 / gamma) @ U.T
    post_cov = np.linalg.inv(prec + np.diag(inv_var.astype(f64)))
    x0 = prng.normal(prng.key(1), (N, D)).astype(f32)
    return StationarityCase(svd, mean, inv_var, x0, post_cov @ (prec @ mean.astype(f64)), np.diag(post_cov).copy(),
                            n_steps)


def stationarity_errors(samples, case: StationarityCase):
    """(max |mean error| / min posterior sd, max |variance ratio - 1|) of samples (..., D) pooled over the rest."""
    s = np.asarray(samples, f64).reshape(-1, case.post_mean.shape[0])
    return (float(np.abs(s.mean(0) - case.post_mean).max() / np.sqrt(case.post_var.min())),
            float(np.abs(s.var(0) / case.post_var - 1.0).max()))


def stationarity_errors_f64(case: StationarityCase, delta: float, seed: int):
    """The fp64 transition on the case, second half kept: (mean error, variance error, mean acceptance)."""
    rng = np.random.default_rng(seed)
    U, gamma = case.cov_svd.U.astype(f64), case.cov_svd.Gamma.astype(f64)
    shift = U @ ((U.T @ case.mean.astype(f64)) / gamma)
    iv = case.inv_var.astype(f64)

    def fn(x):
        return -0.5 * np.sum(iv * x * x, -1) + x @ shift, -(iv * x) + shift

    x = case.x0.astype(f64)
    logp, g = fn(x)
    kept, alphas = [], []
    for t in range(case.n_steps):
        x, logp, g, alpha = transition_f64(rng, x, logp, g, fn, U, gamma, delta)
        if t >= case.n_steps // 2:
            kept.append(x)
            alphas.append(alpha.mean())
    return stationarity_errors(np.stack(kept), case) + (float(np.mean(alphas)),)


# Step size and bounds of the stationarity checks (tests/test_mgrad_gaussian_api.py records how they were measured):
# three times the worst of stationarity_errors_f64(case, 1.0, seed) over seeds 0..4.
STATIONARITY_DELTA = 1.0
STATIONARITY_MEAN_BOUND = 3 * 0.04796
STATIONARITY_VAR_BOUND = 3 * 0.03539
