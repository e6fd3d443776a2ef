"""NumPy restatement of the random-walk Metropolis family (TEST INFRASTRUCTURE, in the style of tests/mala_restatement.py).

Batched with a leading chain axis; chain ``i`` of ``additive_step_kernel(rng_key, state, ...)`` follows the reference's
single-chain ``blackjax.additive_step_random_walk.build_kernel()(jax.random.split(rng_key, N)[chain_offset + i],
state_i, ...)``, and likewise ``rmh_kernel`` / ``irmh_kernel``.

Reference functions followed (cited by name: the reference's source is not held next to this file, so the key split
and the operation order are those of the statement this package was built from, not checked against the source)
* RWState / RWInfo / init, normal,
  build_additive_step, build_rmh
  (transition_energy, kernel, rmh_proposal)   blackjax/mcmc/random_walk.py
* build_kernel                                blackjax/mcmc/irmh.py
* generate_gaussian_noise                     blackjax/util.py
* compute_asymmetric_acceptance_ratio,
  static_binomial_sampling,
  safe_energy_diff                            blackjax/mcmc/proposal.py

One chain:
    key_proposal, key_accept = split(chain_key, 2)
    q1     = q0 + sigma * normal(key_proposal, (D,))      scalar / per-dimension sigma: one fma per element
             q0 + sigma @ normal(key_proposal, (D,))      dense sigma: fp32 fma chain in the engine's k order
                                                          (oracle.fp.gemm_f32chain), one add
             generator(...)                               rmh / irmh: the user's proposal
    e_init = -logp(q0) - f(initial, proposed) ;  e_new = -logp(q1) - f(proposed, initial)       (f: optional)
    delta  = safe_energy_diff(e_init, e_new) ;  p = min(1, exp(delta)) ;  accept = uniform(key_accept) < p
``f(a, b)`` is the log-density of proposing ``b`` from ``a``.

Unlike the reference, generators are batched and receive the transition's ``rng_key`` unchanged (here together with
the per-chain keys, so that a generator can draw ``normal(split(chain_key, 2)[0], (D,))``, the reference's
``key_proposal`` stream).

House numerics: every ``x + s * y`` one fused multiply-add, scalar transcendentals in fp64 rounded
once.  Parity of the random streams with a real JAX run is unpinned, as for the rest of the RNG-dependent surface.
"""
from __future__ import annotations

from typing import Callable, NamedTuple

import numpy as np

from oracle import prng
from oracle.fp import exp_cr, f32, fma32, gemm_f32chain
from oracle.hmc import safe_energy_diff


class RWState(NamedTuple):
    position: np.ndarray  # (N, D)
    logdensity: np.ndarray  # (N,)


class RWInfo(NamedTuple):
    acceptance_rate: np.ndarray  # (N,) float32
    is_accepted: np.ndarray  # (N,) bool
    proposal: RWState


def _value(fn: Callable, q):
    with np.errstate(all="ignore"):
        out = fn(q)
    if isinstance(out, (tuple, list)):
        out = out[0]
    return np.asarray(out, f32)


def init(position, logdensity_fn: Callable) -> RWState:
    position = np.asarray(position, dtype=f32)
    return RWState(position, _value(logdensity_fn, position))


def chain_keys(rng_key, N: int, chain_offset: int = 0, chain_keys_override=None):
    return prng.split(rng_key, N, offset=chain_offset) if chain_keys_override is None else chain_keys_override


def normal(sigma):
    """random_walk.py::normal, batched: ``step(key_proposal (N, 2), position) -> position + move`` (the add is part of
    the step so that the scalar / per-dimension case is one fma, as on the device)."""
    sigma = np.asarray(sigma, dtype=f32)
    if sigma.ndim > 2 or (sigma.ndim == 2 and sigma.shape[0] != sigma.shape[1]):
        raise ValueError(f"sigma must be a scalar, (D,) or (D, D), got {sigma.shape}")

    def step(key_proposal, position):
        N, D = position.shape
        z = prng.normal(key_proposal, (D,))  # generate_gaussian_noise
        with np.errstate(invalid="ignore", over="ignore"):
            if sigma.ndim == 2:
                return (position + gemm_f32chain(z, np.ascontiguousarray(sigma.T))).astype(f32)  # row i: sigma @ z_i
            return fma32(np.broadcast_to(sigma, (D,)).astype(f32), z, position)

    return step


def _finish(kk, state: RWState, q1, logdensity_fn, proposal_logdensity_fn=None, always_accept=False):
    q0, logp0 = state
    q1 = np.asarray(q1, f32)
    logp1 = _value(logdensity_fn, q1)
    proposed = RWState(q1, logp1)
    with np.errstate(invalid="ignore", over="ignore"):
        e_init, e_new = (-logp0).astype(f32), (-logp1).astype(f32)
        if proposal_logdensity_fn is not None:
            e_init = (e_init - np.asarray(proposal_logdensity_fn(state, proposed), f32)).astype(f32)
            e_new = (e_new - np.asarray(proposal_logdensity_fn(proposed, state), f32)).astype(f32)
        delta = safe_energy_diff(e_init, e_new)
        p_acc = np.minimum(exp_cr(delta), f32(1.0))
    acc = prng.uniform(kk[:, 1], ()) < p_acc  # static_binomial_sampling
    if always_accept:  # (the broken sampler the stationarity test must be able to tell from the right one)
        acc = np.ones_like(acc)
    new_state = RWState(np.where(acc[:, None], q1, q0).astype(f32), np.where(acc, logp1, logp0).astype(f32))
    return new_state, RWInfo(p_acc.astype(f32), acc, proposed)


def additive_step_kernel(rng_key, state: RWState, logdensity_fn, random_step, chain_offset: int = 0,
                         chain_keys_override=None, always_accept=False):
    """One transition of every chain.  ``random_step``: what ``normal(sigma)`` returns.  ``chain_keys_override``: (N, 2)
    per-chain keys used instead of ``split(rng_key, .)[chain_offset : chain_offset + N]`` (the chain-major key layout)."""
    kk = prng.split(chain_keys(rng_key, state.position.shape[0], chain_offset, chain_keys_override), 2)
    return _finish(kk, state, random_step(kk[:, 0], state.position), logdensity_fn, always_accept=always_accept)


def rmh_kernel(rng_key, state: RWState, logdensity_fn, transition_generator, proposal_logdensity_fn=None,
               chain_offset: int = 0, chain_keys_override=None):
    """``transition_generator(rng_key, keys (N, 2), position) -> (N, D)``: the per-chain keys are handed over next to
    the unchanged ``rng_key``."""
    keys = chain_keys(rng_key, state.position.shape[0], chain_offset, chain_keys_override)
    q1 = transition_generator(rng_key, keys, state.position)
    return _finish(prng.split(keys, 2), state, q1, logdensity_fn, proposal_logdensity_fn)


def irmh_kernel(rng_key, state: RWState, logdensity_fn, proposal_distribution, proposal_logdensity_fn=None,
                chain_offset: int = 0, chain_keys_override=None):
    """``proposal_distribution(rng_key, keys (N, 2)) -> (N, D)``."""
    keys = chain_keys(rng_key, state.position.shape[0], chain_offset, chain_keys_override)
    q1 = proposal_distribution(rng_key, keys)
    return _finish(prng.split(keys, 2), state, q1, logdensity_fn, proposal_logdensity_fn)


def chain_normal(keys, dim: int, child=None):
    """What ``blackjax_amd.random.chain_normal`` draws, from explicit per-chain keys."""
    k = keys if child is None else prng.split(keys, 2)[:, int(child)]
    return prng.normal(k, (dim,))
