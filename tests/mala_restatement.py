"""NumPy restatement of the MALA transition (TEST INFRASTRUCTURE, in the style of oracle/ghmc.py).

Batched with a leading chain axis; chain ``i`` of ``kernel(rng_key, state, ...)`` follows the reference's
single-chain ``blackjax.mala.build_kernel()(jax.random.split(rng_key, N)[chain_offset + i], state_i, ...)``.

Reference functions followed (cited by name: the reference's source is not held next to this file)
* MALAState / MALAInfo / init           blackjax/mcmc/mala.py
* transition_energy, kernel             blackjax/mcmc/mala.py (build_kernel)
* overdamped_langevin one_step          blackjax/mcmc/diffusions.py
* generate_gaussian_noise               blackjax/util.py
* compute_asymmetric_acceptance_ratio,
  static_binomial_sampling,
  safe_energy_diff                      blackjax/mcmc/proposal.py

House numerics: every ``x + s * y`` one fused multiply-add, reductions over D in fp64
rounded once, scalar transcendentals in fp64 rounded once.  Parity of the random streams with a real JAX run
is unpinned, as for the rest of the RNG-dependent surface.
"""
from __future__ import annotations

from typing import Callable, NamedTuple

import numpy as np

from oracle import prng
from oracle.fp import dot64, exp_cr, f32, fma32, sqrt32
from oracle.hmc import safe_energy_diff


class MALAState(NamedTuple):
    position: np.ndarray  # (N, D)
    logdensity: np.ndarray  # (N,)
    logdensity_grad: np.ndarray  # (N, D)


class MALAInfo(NamedTuple):
    acceptance_rate: np.ndarray  # (N,) float32
    is_accepted: np.ndarray  # (N,) bool


def init(position, logdensity_fn: Callable) -> MALAState:
    position = np.asarray(position, dtype=f32)
    logp, grad = logdensity_fn(position)
    return MALAState(position, np.asarray(logp, f32), np.asarray(grad, f32))


def _transition_energy(q_from, q_to, logp_to, g_to, tau_col, c):
    """transition_energy(state, new_state) = -logp(new) + 0.25 * (1 / tau) * |q - q_new - tau * g_new|^2."""
    with np.errstate(invalid="ignore", over="ignore"):
        theta = fma32(-tau_col, g_to, (q_from - q_to).astype(f32))
        return fma32(c, dot64(theta, theta), -np.asarray(logp_to, f32))


def kernel(rng_key, state: MALAState, logdensity_fn, step_size, chain_offset: int = 0, chain_keys_override=None):
    """One transition of every chain.  ``step_size``: a scalar or (N,).  ``chain_keys_override``: (N, 2) per-chain
    keys used instead of ``split(rng_key, .)[chain_offset : chain_offset + N]`` (the chain-major key layout)."""
    q0, logp0, g0 = state
    N, D = q0.shape
    tau = np.broadcast_to(np.asarray(step_size, dtype=f32), (N,)).astype(f32)
    tau_col = tau[:, None]
    keys = prng.split(rng_key, N, offset=chain_offset) if chain_keys_override is None else chain_keys_override
    kk = prng.split(keys, 2)  # key_integrator, key_rmh
    noise = prng.normal(kk[:, 0], (D,))  # generate_gaussian_noise
    s = sqrt32((f32(2.0) * tau_col).astype(f32))
    with np.errstate(invalid="ignore", over="ignore"):
        q1 = fma32(s, noise, fma32(tau_col, g0, q0))  # p + tau * g + sqrt(2 tau) * n, left to right
    with np.errstate(all="ignore"):
        logp1, g1 = logdensity_fn(q1)
    logp1, g1 = np.asarray(logp1, f32), np.asarray(g1, f32)
    c = (f32(0.25) * (f32(1.0) / tau).astype(f32)).astype(f32)  # two fp32 roundings, as written in mala.py
    e_new = _transition_energy(q0, q1, logp1, g1, tau_col, c)   # transition_energy(state, new_state)
    e_prev = _transition_energy(q1, q0, logp0, g0, tau_col, c)  # transition_energy(new_state, state)
    delta = safe_energy_diff(e_prev, e_new)
    p_acc = np.minimum(exp_cr(delta), f32(1.0))
    acc = prng.uniform(kk[:, 1], ()) < p_acc  # static_binomial_sampling
    am = acc[:, None]
    new_state = MALAState(np.where(am, q1, q0).astype(f32), np.where(acc, logp1, logp0).astype(f32),
                          np.where(am, g1, g0).astype(f32))
    return new_state, MALAInfo(p_acc.astype(f32), acc)
