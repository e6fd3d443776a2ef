"""NumPy restatement of the Barker-proposal transition (TEST INFRASTRUCTURE, in the style of tests/mala_restatement.py).

Batched with a leading chain axis; chain ``i`` of ``kernel(rng_key, state, ...)`` follows the reference's
single-chain ``blackjax.barker_proposal.build_kernel()(jax.random.split(rng_key, N)[chain_offset + i], state_i, ...)``
with a diagonal preconditioner.

Reference functions followed (cited by name: the reference's source is not held next to this file)
* BarkerState / BarkerInfo / init       blackjax/mcmc/barker.py
* _barker_sample_nd, _barker_logpdf,
  kernel                                blackjax/mcmc/barker.py (build_kernel)
* compute_asymmetric_acceptance_ratio,
  static_binomial_sampling,
  safe_energy_diff                      blackjax/mcmc/proposal.py

House numerics: every fp32 product and sum one rounding, reductions over D in fp64 rounded
once, transcendentals in fp64 rounded once.  With a diagonal scale sigma the log-density of the proposal depends on
(y - x)_d / sigma_d * sigma_d g_d = (y - x)_d g_d only, so the accept needs neither the step size nor the metric.
Parity of the random streams with a real JAX run is unpinned, as for the rest of the RNG-dependent surface.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from oracle import prng
from oracle.fp import exp_cr, expit_cr, f32, f64, sqrt32
from oracle.hmc import safe_energy_diff


class BarkerState(NamedTuple):
    position: np.ndarray  # (N, D)
    logdensity: np.ndarray  # (N,)
    logdensity_grad: np.ndarray  # (N, D)


class BarkerInfo(NamedTuple):
    acceptance_rate: np.ndarray  # (N,) float32
    is_accepted: np.ndarray  # (N,) bool
    proposal: BarkerState


def init(position, logdensity_fn) -> BarkerState:
    position = np.asarray(position, dtype=f32)
    logp, grad = logdensity_fn(position)
    return BarkerState(position, np.asarray(logp, f32), np.asarray(grad, f32))


def softplus64(x):
    """softplus(x) = max(x, 0) + log1p(exp(-|x|)) in fp64 (fp32 argument, fp64 result)."""
    x = np.asarray(x, dtype=f32).astype(f64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def chain_keys(rng_key, n, chain_offset=0, chain_keys_override=None):
    return prng.split(rng_key, n, offset=chain_offset) if chain_keys_override is None else chain_keys_override


def propose(keys, q0, g0, step_size, inverse_mass_matrix=None):
    """_barker_sample_nd for the (N, 2) chain keys: -> (q1, b, z), the proposal, the per-element signs (True: +z)
    and the increments."""
    N, D = q0.shape
    tau_col = np.broadcast_to(np.asarray(step_size, dtype=f32), (N,)).astype(f32)[:, None]
    imm = np.ones(D, f32) if inverse_mass_matrix is None else np.asarray(inverse_mass_matrix, dtype=f32)
    ks = prng.split(keys, 2)[:, 0]  # key_sample, key_rmh = split(chain key)
    k12 = prng.split(ks, 2)  # k1, k2
    n = prng.normal(k12[:, 0], (D,))
    u = prng.uniform(k12[:, 1], (D,))
    with np.errstate(invalid="ignore", over="ignore"):
        s = (tau_col * sqrt32(imm)).astype(f32)
        z = (s * n).astype(f32)
        c = (z * g0).astype(f32)
        p = expit_cr(c)
        b = u < p  # a NaN p compares false
        q1 = np.where(b, (q0 + z).astype(f32), (q0 - z).astype(f32)).astype(f32)
    return q1, b, z


def kernel(rng_key, state: BarkerState, logdensity_fn, step_size, inverse_mass_matrix=None, chain_offset: int = 0,
           chain_keys_override=None):
    """One transition of every chain.  ``step_size``: a scalar or (N,).  ``inverse_mass_matrix``: None (ones), (D,)
    or (N, D).  ``chain_keys_override``: (N, 2) per-chain keys used instead of
    ``split(rng_key, .)[chain_offset : chain_offset + N]`` (the chain-major key layout)."""
    q0, logp0, g0 = state
    N, D = q0.shape
    keys = chain_keys(rng_key, N, chain_offset, chain_keys_override)
    q1, _, _ = propose(keys, q0, g0, step_size, inverse_mass_matrix)
    with np.errstate(all="ignore"):
        logp1, g1 = logdensity_fn(q1)
    logp1, g1 = np.asarray(logp1, f32), np.asarray(g1, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (q1 - q0).astype(f32)
        a = (-(t * g0).astype(f32)).astype(f32)
        e = (t * g1).astype(f32)
        S = np.sum(softplus64(a) - softplus64(e), axis=-1).astype(f32)  # fp64 sum, rounded once
        log_ratio = safe_energy_diff((logp1 - logp0).astype(f32), -S)  # (logp1 - logp0) + S, NaN -> -inf
    p_acc = np.minimum(exp_cr(log_ratio), f32(1.0))
    acc = prng.uniform(prng.split(keys, 2)[:, 1], ()) < p_acc  # static_binomial_sampling
    am = acc[:, None]
    new_state = BarkerState(np.where(am, q1, q0).astype(f32), np.where(acc, logp1, logp0).astype(f32),
                            np.where(am, g1, g0).astype(f32))
    return new_state, BarkerInfo(p_acc.astype(f32), acc, BarkerState(q1, logp1, g1))
