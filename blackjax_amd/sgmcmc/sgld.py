"""Batched stochastic gradient Langevin dynamics on MI355X behind the ``blackjax.sgld`` API surface.

Mirrors blackjax/sgmcmc/sgld.py: ``init``, ``build_kernel`` and ``as_top_level_api``; the update is one step of
sgmcmc/diffusions.py::overdamped_langevin with the chain's key itself drawing the noise.  The state is the position
tensor.  A transition is the user's ``grad_estimator(position, minibatch)`` (one autograd pass; never traced, since
the minibatch changes every step) followed by ONE launch, ``bjx_sgld_step`` (include/bjx_hip.h, "SGMCMC").

The chain axis is native; chain ``i`` of ``step(rng_key, position, minibatch, step_size)`` reproduces the reference's
single-chain ``step(jax.random.split(rng_key, N)[chain_offset + i], position_i, minibatch, step_size)``.
``step_size`` and ``temperature`` may be per-chain ``(N,)`` tensors (a replica ladder in one batch) and arrive with
every call, as schedules change them.  Like every RNG-dependent part of the package, parity with a real JAX run is
unpinned; the arithmetic is held against a NumPy restatement of the reference
(tests/sgmcmc_restatement.py).
"""
from __future__ import annotations

from typing import Callable

import torch

from .._util import check_batch
from ..base import SamplingAlgorithm
from . import diffusions

__all__ = ["init", "build_kernel", "as_top_level_api"]


def init(position: torch.Tensor) -> torch.Tensor:
    """blackjax/sgmcmc/sgld.py ``init``: the state is the position."""
    position = check_batch(position, "position")
    if position.ndim != 2:
        raise ValueError(f"position must be (n_chains, dim), got {tuple(position.shape)}")
    return position


def build_kernel():
    """blackjax/sgmcmc/sgld.py ``build_kernel``."""
    integrator = diffusions.overdamped_langevin()

    def kernel(rng_key, position, grad_estimator: Callable, minibatch, step_size, temperature=1.0, *,
               chain_offset: int = 0):
        q, _, _ = diffusions._batch_args(position, step_size, temperature)
        g = diffusions.estimate_gradient(grad_estimator, q, minibatch)
        return integrator(rng_key, q, g, step_size, temperature, chain_offset=chain_offset)

    return kernel


def as_top_level_api(grad_estimator: Callable, *, chain_offset: int = 0) -> SamplingAlgorithm:
    """blackjax/sgmcmc/sgld.py ``as_top_level_api``: ``init(position)``,
    ``step(rng_key, state, minibatch, step_size, temperature=1.0)``."""
    kernel = build_kernel()

    def init_fn(position, rng_key=None):
        del rng_key
        return init(position)

    def step_fn(rng_key, state, minibatch, step_size, temperature=1.0):
        return kernel(rng_key, state, grad_estimator, minibatch, step_size, temperature, chain_offset=chain_offset)

    return SamplingAlgorithm(init_fn, step_fn)
