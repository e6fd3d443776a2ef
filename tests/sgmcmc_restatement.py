"""NumPy restatement of the stochastic-gradient samplers (TEST INFRASTRUCTURE, in the style of tests/mala_restatement.py).

Batched with a leading chain axis; chain ``i`` of ``*_kernel(rng_key, ...)`` follows the reference's single-chain
kernel called with ``jax.random.split(rng_key, N)[chain_offset + i]``.

Reference functions followed (cited by name: the reference's source is not held next to this file)
* init, kernel                          blackjax/sgmcmc/sgld.py, blackjax/sgmcmc/sghmc.py, blackjax/sgmcmc/sgnht.py
* overdamped_langevin, sghmc, sgnht     blackjax/sgmcmc/diffusions.py
* logdensity_estimator, grad_estimator,
  control_variates                      blackjax/sgmcmc/gradients.py
* generate_gaussian_noise               blackjax/util.py

House numerics: every ``x + s * y`` one fused multiply-add, scalars in fp32 in the order written,
the reduction over D in fp64 rounded once.  Parity of the random streams with a real JAX run is unpinned, as for the
rest of the RNG-dependent surface.

A ``grad_estimator`` here is any callable ``(position (N, D), minibatch) -> (N, D)`` over NumPy arrays.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from oracle import prng
from oracle.fp import f32, fma32, sqrt32


def _per_chain(x, N):
    return np.broadcast_to(np.asarray(x, dtype=f32), (N,)).astype(f32)[:, None]


def _chain_keys(rng_key, N, chain_offset, chain_keys_override):
    return prng.split(rng_key, N, offset=chain_offset) if chain_keys_override is None else chain_keys_override


def _friction_noise_scale(eps, T, alpha, beta):
    """sqrt(eps * T * (2 alpha - eps beta)) in fp32, in this order (diffusions.py sghmc / sgnht)."""
    alpha, beta = f32(alpha), f32(beta)
    with np.errstate(invalid="ignore"):
        return sqrt32(((eps * T).astype(f32) * (f32(2.0) * alpha - (eps * beta).astype(f32)).astype(f32)).astype(f32))


def sgld_kernel(rng_key, position, grad_estimator, minibatch, step_size, temperature=1.0, chain_offset: int = 0,
                chain_keys_override=None):
    """sgld.py kernel + diffusions.py overdamped_langevin: q + eps g + sqrt(2 T eps) normal(chain key)."""
    q = np.asarray(position, f32)
    N, D = q.shape
    eps, T = _per_chain(step_size, N), _per_chain(temperature, N)
    keys = _chain_keys(rng_key, N, chain_offset, chain_keys_override)
    g = np.asarray(grad_estimator(q, minibatch), f32)
    z = prng.normal(keys, (D,))
    s = sqrt32(((f32(2.0) * T).astype(f32) * eps).astype(f32))
    with np.errstate(invalid="ignore", over="ignore"):
        return fma32(s, z, fma32(eps, g, q))


def sghmc_kernel(rng_key, position, grad_estimator, minibatch, step_size, num_integration_steps, temperature=1.0,
                 alpha=0.01, beta=0.0, chain_offset: int = 0, chain_keys_override=None, return_momentum=False):
    """sghmc.py kernel + diffusions.py sghmc, all ``num_integration_steps`` steps in full (the estimator is called L
    times; the last call only feeds the dropped momentum)."""
    q = np.asarray(position, f32)
    N, D = q.shape
    L = int(num_integration_steps)
    eps, T = _per_chain(step_size, N), _per_chain(temperature, N)
    keys = _chain_keys(rng_key, N, chain_offset, chain_keys_override)
    p = prng.normal(keys, (D,))  # momentum refresh with the chain key itself
    step_keys = prng.split(keys, L)  # (N, L, 2)
    c = (f32(1.0) - (f32(alpha) * eps).astype(f32)).astype(f32)  # two fp32 roundings
    s = _friction_noise_scale(eps, T, alpha, beta)
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(L):
            g = np.asarray(grad_estimator(q, minibatch), f32)
            z = prng.normal(step_keys[:, l], (D,))
            q_next = fma32(eps, p, q)
            p = fma32(s, z, fma32(eps, g, (c * p).astype(f32)))
            q = q_next
    return (q, p) if return_momentum else q


class SGNHTState(NamedTuple):
    position: np.ndarray  # (N, D)
    momentum: np.ndarray  # (N, D)
    xi: np.ndarray  # (N,)


def sgnht_init(position, rng_key, xi, chain_offset: int = 0, chain_keys_override=None) -> SGNHTState:
    q = np.asarray(position, f32)
    N, D = q.shape
    keys = _chain_keys(rng_key, N, chain_offset, chain_keys_override)
    return SGNHTState(q, prng.normal(keys, (D,)), np.broadcast_to(np.asarray(xi, f32), (N,)).astype(f32))


def sgnht_kernel(rng_key, state: SGNHTState, grad_estimator, minibatch, step_size, temperature=1.0, alpha=0.01,
                 beta=0.0, chain_offset: int = 0, chain_keys_override=None) -> SGNHTState:
    """sgnht.py kernel + diffusions.py sgnht."""
    q, p, xi = (np.asarray(x, f32) for x in state)
    N, D = q.shape
    eps, T = _per_chain(step_size, N), _per_chain(temperature, N)
    keys = _chain_keys(rng_key, N, chain_offset, chain_keys_override)
    g = np.asarray(grad_estimator(q, minibatch), f32)
    z = prng.normal(keys, (D,))
    s = _friction_noise_scale(eps, T, alpha, beta)
    with np.errstate(invalid="ignore", over="ignore"):
        q1 = fma32(eps, p, q)
        t = fma32(-(eps * xi[:, None]).astype(f32), p, p)
        t = fma32(eps, g, t)
        p1 = fma32(s, z, t)
        m = (np.sum(p1.astype(np.float64) ** 2, axis=-1) / D).astype(f32)  # fp64 accumulation, rounded once
        xi1 = fma32(eps[:, 0], (m - T[:, 0]).astype(f32), xi)
    return SGNHTState(q1, p1, xi1)


# ---- gradients.py on the Gaussian-mean model, in closed form ---------------------------------------------------------
# prior q ~ N(0, s0^2 I); data y_b ~ N(q, I), b < M: log p(y_b | q) = -|y_b - q|^2 / 2 (+ const).  A minibatch is
# (B, D), shared by the chains, or (N, B, D), one per chain.

def gaussian_mean_logdensity_estimator(prior_sd, data_size):
    """gradients.py logdensity_estimator: logprior(q) + data_size * mean_b loglikelihood(q, y_b), in float64."""
    def f(position, minibatch):
        q = np.asarray(position, np.float64)
        y = np.asarray(minibatch, np.float64)
        y = y[None] if y.ndim == 2 else y
        loglik = -0.5 * ((y - q[:, None, :]) ** 2).sum(-1)  # (N, B)
        return -0.5 * (q * q).sum(-1) / prior_sd ** 2 + data_size * loglik.mean(-1)

    return f


def gaussian_mean_grad_estimator(prior_sd, data_size):
    """gradients.py grad_estimator, the gradient of the above: -q / s0^2 + (M / B) sum_b (y_b - q), in float64
    rounded once to fp32."""
    def f(position, minibatch):
        q = np.asarray(position, np.float64)
        y = np.asarray(minibatch)
        y = y[None] if y.ndim == 2 else y
        B = y.shape[1]
        return (-q / prior_sd ** 2 + (data_size / B) * (y.sum(1, dtype=np.float64) - B * q)).astype(f32)

    return f


def control_variates(logdensity_grad_estimator, centering_position, data):
    """gradients.py control_variates: the full-data gradient at the centre, evaluated once, plus the minibatch
    difference between the position and the centre."""
    centre = np.asarray(centering_position, f32)
    centre = centre[None] if centre.ndim == 1 else centre
    cv_grad_value = logdensity_grad_estimator(centre, data)

    def f(position, minibatch):
        return (cv_grad_value + logdensity_grad_estimator(position, minibatch)
                - logdensity_grad_estimator(centre, minibatch)).astype(f32)

    return f


# ---- what the sampler tests expect, from the linear recursion of the restated arithmetic (float64) -------------------

def sghmc_stationary_variance(step_size, alpha, beta, num_integration_steps, temperature):
    """Stationary position variance of ``sghmc_kernel`` on the target N(0, 1) with the exact gradient g = -q.  One
    kernel call maps the position variance v to v': from Sigma = diag(v, 1) (the momentum is refreshed to N(0, 1)),
    L - 1 steps Sigma <- A Sigma A^T + Q with A = [[1, eps], [-eps, c]], Q = diag(0, s^2), then the position-only step
    v' = Sigma_qq + 2 eps Sigma_qp + eps^2 Sigma_pp.  The map is affine, so two evaluations give its fixed point.
    Returns (fixed point, contraction per call)."""
    eps, T = float(step_size), float(temperature)
    c = 1.0 - alpha * eps
    s2 = eps * T * (2.0 * alpha - eps * beta)
    A = np.array([[1.0, eps], [-eps, c]])
    Q = np.diag([0.0, s2])

    def call(v):
        S = np.diag([v, 1.0])
        for _ in range(int(num_integration_steps) - 1):
            S = A @ S @ A.T + Q
        return S[0, 0] + 2.0 * eps * S[0, 1] + eps * eps * S[1, 1]

    b = call(0.0)
    a = call(1.0) - b
    return b / (1.0 - a), a
