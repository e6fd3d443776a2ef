"""NumPy restatement of the elliptical slice transition (TEST INFRASTRUCTURE, in the style of tests/mala_restatement.py).

Batched with a leading chain axis; chain ``i`` of ``kernel(rng_key, state, ...)`` follows the reference's
single-chain ``blackjax.elliptical_slice.build_kernel(cov, mean)(jax.random.split(rng_key, N)[chain_offset + i],
state_i, loglikelihood_fn)``.

Reference functions followed (cited by name: the reference's source is not held next to this file, so the key split
and the operation order are those of the statement this package was built from, not checked against the source)
* EllipSliceState / EllipSliceInfo / init     blackjax/mcmc/elliptical_slice.py
* kernel, elliptical_proposal (generate,
  slice_fn and its while_loop), ellipsis      blackjax/mcmc/elliptical_slice.py
* generate_gaussian_noise                     blackjax/util.py

One chain:
    key_slice, key_momentum, key_uniform, key_theta = split(chain_key, 4)
    nu    = mean + sqrt(cov) * normal(key_momentum, (D,))       diagonal cov: one fma per element
            mean + (L normal(...))                              dense cov: L = cholesky(cov), fp32 fma chain in the
                                                                engine's k order (oracle.fp.gemm_f32chain), one add
    logy  = logdensity + log(uniform(key_uniform))
    theta = 2 pi uniform(key_theta); theta_min = theta - 2 pi; theta_max = theta
    p, m  = ellipsis(theta); logp = loglikelihood(p); subiter = 1
    while logp <= logy:                                         (literally: a NaN logp ends the loop)
        theta = uniform(fold_in(key_slice, subiter), minval=theta_min, maxval=theta_max)
        p, m = ellipsis(theta); logp = loglikelihood(p)
        theta_min = theta if theta < 0 else theta_min; theta_max = theta if theta > 0 else theta_max
        subiter += 1
    ellipsis(theta): a = q0 - mean; b = nu - mean; p = a cos(theta) + b sin(theta) + mean; m = b cos - a sin + mean

House numerics: every ``x + s * y`` one fused multiply-add, scalar transcendentals (log, cos,
sin) in fp64 rounded once.  The one deliberate difference from the reference is the cap: the loop raises after
``max_subiter`` likelihood evaluations instead of running for ever.  Parity of the random streams with a real JAX run
is unpinned, as for the rest of the RNG-dependent surface.
"""
from __future__ import annotations

from typing import Callable, NamedTuple

import numpy as np

from oracle import prng
from oracle.fp import f32, fma32, gemm_f32chain, log_cr, sqrt32

TWO_PI = f32(2.0 * np.pi)


class EllipSliceState(NamedTuple):
    position: np.ndarray  # (N, D)
    logdensity: np.ndarray  # (N,)


class EllipSliceInfo(NamedTuple):
    momentum: np.ndarray  # (N, D) float32
    theta: np.ndarray  # (N,) float32
    subiter: np.ndarray  # (N,) int32


def _loglik(fn: Callable, q):
    with np.errstate(all="ignore"):
        out = fn(q)
    if isinstance(out, (tuple, list)):
        out = out[0]
    return np.asarray(out, f32)


def init(position, loglikelihood_fn: Callable) -> EllipSliceState:
    position = np.asarray(position, dtype=f32)
    return EllipSliceState(position, _loglik(loglikelihood_fn, position))


def cholesky_t(cov) -> np.ndarray:
    """L^T of a dense ``cov``, L = cholesky(cov) in fp64 rounded once to fp32 (row-major (D, D))."""
    return np.ascontiguousarray(np.linalg.cholesky(np.asarray(cov, np.float64)).astype(f32).T)


def _ellipsis(q0, nu, mean, theta):
    """Both points of the ellipse at ``theta`` (N,): cos / sin in fp64 rounded once."""
    c = np.cos(theta.astype(np.float64)).astype(f32)[:, None]
    s = np.sin(theta.astype(np.float64)).astype(f32)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        a = (q0 - mean).astype(f32)
        b = (nu - mean).astype(f32)
        p = (fma32(b, s, (a * c).astype(f32)) + mean).astype(f32)
        m = (fma32(-a, s, (b * c).astype(f32)) + mean).astype(f32)
    return p, m


def kernel(rng_key, state: EllipSliceState, loglikelihood_fn, *, mean, cov, chain_offset: int = 0,
           chain_keys_override=None, chol_t=None, max_subiter: int = 1024):
    """One transition of every chain.  ``mean``: scalar or (D,); ``cov``: (D,) diagonal or (D, D) dense.
    ``chain_keys_override``: (N, 2) per-chain keys used instead of ``split(rng_key, .)[chain_offset : chain_offset + N]``
    (the chain-major key layout).  ``chol_t``: the fp32 factor L^T to use for a dense ``cov`` instead of
    ``cholesky_t(cov)`` (two fp64 LAPACK builds may round a few of its entries differently)."""
    q0, logp0 = state
    N, D = q0.shape
    mean = np.broadcast_to(np.asarray(mean, dtype=f32), (D,)).astype(f32)
    cov = np.asarray(cov, dtype=f32)
    keys = prng.split(rng_key, N, offset=chain_offset) if chain_keys_override is None else chain_keys_override
    kk = prng.split(keys, 4)  # key_slice, key_momentum, key_uniform, key_theta
    k_slice = kk[:, 0]
    n = prng.normal(kk[:, 1], (D,))  # generate_gaussian_noise
    if cov.ndim == 1:
        nu = fma32(sqrt32(cov), n, mean)
    else:
        lt = cholesky_t(cov) if chol_t is None else np.asarray(chol_t, f32)
        nu = (gemm_f32chain(n, lt) + mean).astype(f32)
    with np.errstate(invalid="ignore"):
        logy = (logp0 + log_cr(prng.uniform(kk[:, 2], ()))).astype(f32)
    theta = (TWO_PI * prng.uniform(kk[:, 3], ())).astype(f32)
    theta_min = (theta - TWO_PI).astype(f32)
    theta_max = theta.copy()
    p, m = _ellipsis(q0, nu, mean, theta)
    logp = _loglik(loglikelihood_fn, p)
    subiter = np.ones(N, np.int32)
    evals = 1
    while True:
        live = logp <= logy  # the reference's loop condition, per chain
        if not live.any():
            break
        if evals >= max_subiter:
            raise RuntimeError(f"{int(live.sum())} of {N} chains still live after {max_subiter} evaluations")
        idx = np.nonzero(live)[0]
        f = prng.bits_to_unit_float(prng.random_bits(prng.fold_in(k_slice[idx], subiter[idx].astype(np.uint32)), ()))
        lo, hi = theta_min[idx], theta_max[idx]
        th = np.maximum(lo, fma32(f, (hi - lo).astype(f32), lo))  # oracle.prng.uniform with per-chain bounds
        p_i, m_i = _ellipsis(q0[idx], nu[idx], mean, th)
        p[idx], m[idx], theta[idx] = p_i, m_i, th
        logp[idx] = _loglik(loglikelihood_fn, p)[idx]
        theta_min[idx] = np.where(th < 0, th, lo)
        theta_max[idx] = np.where(th > 0, th, hi)
        subiter[idx] += 1
        evals += 1
    return EllipSliceState(p, logp), EllipSliceInfo(m, theta, subiter)


# ------------------------------------------------------------------ the conjugate case of the stationarity tests
# (tests/test_elliptical_slice_api.py on the restatement, tests/test_elliptical_slice_gpu.py on the device): Gaussian
# prior N(MEAN, diag(COV)), likelihood exp(-0.5 sum PREC (q - OBS)^2); the posterior is Gaussian with precision
# 1 / COV + PREC.
MEAN = np.array([1.5, -2.0, 0.0, 4.0])
COV = np.array([0.25, 1.0, 4.0, 9.0])
OBS = np.array([0.5, 0.5, -1.0, 2.0])
PREC = np.array([4.0, 1.0, 0.25, 2.0])
VAR_POST = 1.0 / (1.0 / COV + PREC)
MEAN_POST = VAR_POST * (MEAN / COV + PREC * OBS)


def conjugate_loglik(q):
    d = np.asarray(q, np.float64) - OBS
    return (-0.5 * np.sum(PREC * d * d, axis=-1)).astype(f32)


def posterior_draws(N):
    return (MEAN_POST + np.sqrt(VAR_POST) * np.random.default_rng(0).standard_normal((N, 4))).astype(f32)


def moment_errors(x):
    """|mean - posterior mean| and |var - posterior var| of the ensemble in standard errors of N independent draws."""
    x = np.asarray(x, np.float64)
    N = x.shape[0]
    mean_se = np.abs(x.mean(0) - MEAN_POST) / np.sqrt(VAR_POST / N)
    var_se = np.abs(x.var(0, ddof=1) - VAR_POST) / (VAR_POST * np.sqrt(2.0 / (N - 1)))
    return mean_se, var_se
