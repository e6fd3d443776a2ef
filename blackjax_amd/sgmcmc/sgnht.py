"""Batched stochastic gradient Nose-Hoover thermostat on MI355X behind the ``blackjax.sgnht`` API surface.

Mirrors blackjax/sgmcmc/sgnht.py: ``SGNHTState``, ``init``, ``build_kernel(alpha, beta)`` and ``as_top_level_api``;
the update is one step of sgmcmc/diffusions.py::sgnht with the chain's key itself drawing the noise.  A transition is
the user's ``grad_estimator(position, minibatch)`` followed by ONE launch, ``bjx_sgnht_step`` (include/bjx_hip.h,
"SGMCMC"), which also reduces the new momentum's mean square for the thermostat.

The chain axis is native; chain ``i`` of a batched call reproduces the reference's single-chain call made with
``jax.random.split(rng_key, N)[chain_offset + i]`` (``init`` included: it draws the momentum).  ``step_size`` and
``temperature`` may be per-chain ``(N,)`` tensors.  Like every RNG-dependent part of the package, parity with a real
JAX run is unpinned; the arithmetic is held against a NumPy restatement of the reference
(tests/sgmcmc_restatement.py).
"""
from __future__ import annotations

from typing import Callable, NamedTuple

import torch

from .._util import check_batch
from ..base import SamplingAlgorithm
from ..random import chain_normal
from . import diffusions

__all__ = ["SGNHTState", "init", "build_kernel", "as_top_level_api"]


class SGNHTState(NamedTuple):
    """blackjax/sgmcmc/sgnht.py ``SGNHTState``, batched: (N, D), (N, D), (N,)."""

    position: torch.Tensor
    momentum: torch.Tensor
    xi: torch.Tensor


def init(position: torch.Tensor, rng_key, xi, *, chain_offset: int = 0) -> SGNHTState:
    """blackjax/sgmcmc/sgnht.py ``init``: ``momentum = normal(kc, (D,))`` per chain; ``xi`` is a float or ``(N,)``."""
    position = check_batch(position, "position")
    if position.ndim != 2:
        raise ValueError(f"position must be (n_chains, dim), got {tuple(position.shape)}")
    N, D = position.shape
    momentum = chain_normal(rng_key, N, D, device=position.device, chain_offset=chain_offset, child=None)
    if isinstance(xi, torch.Tensor) and xi.ndim > 0:
        xi = check_batch(xi, "xi")
        if xi.shape != (N,) or xi.device != position.device:
            raise ValueError(f"xi must be a float or ({N},) on {position.device}, got {tuple(xi.shape)} on {xi.device}")
    else:
        xi = torch.full((N,), float(xi), dtype=torch.float32, device=position.device)
    return SGNHTState(position, momentum, xi)


def build_kernel(alpha: float = 0.01, beta: float = 0.0):
    """blackjax/sgmcmc/sgnht.py ``build_kernel``."""
    integrator = diffusions.sgnht(alpha, beta)

    def kernel(rng_key, state: SGNHTState, grad_estimator: Callable, minibatch, step_size, temperature=1.0, *,
               chain_offset: int = 0) -> SGNHTState:
        diffusions.check_friction(step_size, alpha, beta)
        position, momentum, xi = state
        q, _, _ = diffusions._batch_args(position, step_size, temperature, "state.position")
        g = diffusions.estimate_gradient(grad_estimator, q, minibatch)
        return SGNHTState(*integrator(rng_key, q, momentum, xi, g, step_size, temperature,
                                      chain_offset=chain_offset))

    return kernel


def as_top_level_api(grad_estimator: Callable, alpha: float = 0.01, beta: float = 0.0, *,
                     chain_offset: int = 0) -> SamplingAlgorithm:
    """blackjax/sgmcmc/sgnht.py ``as_top_level_api``: ``init(position, rng_key, init_xi=None)`` (``None``: ``alpha``),
    ``step(rng_key, state, minibatch, step_size, temperature=1.0)``."""
    kernel = build_kernel(alpha, beta)

    def init_fn(position, rng_key, init_xi=None):
        return init(position, rng_key, alpha if init_xi is None else init_xi, chain_offset=chain_offset)

    def step_fn(rng_key, state, minibatch, step_size, temperature=1.0):
        return kernel(rng_key, state, grad_estimator, minibatch, step_size, temperature, chain_offset=chain_offset)

    return SamplingAlgorithm(init_fn, step_fn)
