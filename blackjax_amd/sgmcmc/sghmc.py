"""Batched stochastic gradient Hamiltonian Monte Carlo on MI355X behind the ``blackjax.sghmc`` API surface.

Mirrors blackjax/sgmcmc/sghmc.py: ``init``, ``build_kernel(alpha, beta)`` and ``as_top_level_api``; a transition
refreshes the momentum with the chain's key, ``normal(kc, (D,))``, and takes ``num_integration_steps`` steps of
sgmcmc/diffusions.py::sghmc with the keys ``split(kc, num_integration_steps)``; the result is the last position, the
momentum is dropped.  The state is the position tensor.

Each integration step is the user's ``grad_estimator(position, minibatch)`` followed by one launch of
``bjx_sghmc_step`` (include/bjx_hip.h, "SGMCMC").  The first launch draws the refreshed momentum in registers: there
is no launch and no tensor for the refresh.  The gradient and the noise of the LAST step feed only the final momentum,
which nobody reads, so the driver does not call the estimator for that step and the last launch writes only the
position: the result is identical, at ``num_integration_steps - 1`` gradient passes per transition instead of
``num_integration_steps``.  An estimator with side effects therefore sees one call fewer than in the reference.

The chain axis is native; chain ``i`` of a batched call reproduces the reference's single-chain call made with
``jax.random.split(rng_key, N)[chain_offset + i]``.  ``step_size`` and ``temperature`` may be per-chain ``(N,)``
tensors.  Like every RNG-dependent part of the package, parity with a real JAX run is unpinned;
the arithmetic is held against a NumPy restatement of the reference (tests/sgmcmc_restatement.py).
"""
from __future__ import annotations

from typing import Callable

from ..base import SamplingAlgorithm
from . import diffusions
from .sgld import init

__all__ = ["init", "build_kernel", "as_top_level_api"]


def build_kernel(alpha: float = 0.01, beta: float = 0.0):
    """blackjax/sgmcmc/sghmc.py ``build_kernel``."""
    integrator = diffusions.sghmc(alpha, beta)

    def kernel(rng_key, position, grad_estimator: Callable, minibatch, step_size, num_integration_steps,
               temperature=1.0, *, chain_offset: int = 0):
        L = int(num_integration_steps)
        if L < 1:
            raise ValueError(f"num_integration_steps must be at least 1, got {num_integration_steps}")
        diffusions.check_friction(step_size, alpha, beta)
        q, _, _ = diffusions._batch_args(position, step_size, temperature)
        p = None  # the first launch draws the refreshed momentum itself
        for step in range(L):
            # the last step's gradient would feed only the dropped momentum: not evaluated
            g = diffusions.estimate_gradient(grad_estimator, q, minibatch) if step < L - 1 else None
            q, p = integrator(rng_key, q, p, g, step_size, temperature, chain_offset=chain_offset, step_index=step)
        return q

    return kernel


def as_top_level_api(grad_estimator: Callable, num_integration_steps: int = 10, alpha: float = 0.01,
                     beta: float = 0.0, *, chain_offset: int = 0) -> SamplingAlgorithm:
    """blackjax/sgmcmc/sghmc.py ``as_top_level_api``: ``init(position)``,
    ``step(rng_key, state, minibatch, step_size, temperature=1.0)``."""
    kernel = build_kernel(alpha, beta)

    def init_fn(position, rng_key=None):
        del rng_key
        return init(position)

    def step_fn(rng_key, state, minibatch, step_size, temperature=1.0):
        return kernel(rng_key, state, grad_estimator, minibatch, step_size, num_integration_steps, temperature,
                      chain_offset=chain_offset)

    return SamplingAlgorithm(init_fn, step_fn)
