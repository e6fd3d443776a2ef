"""Effective sample size behind ``blackjax.smc.ess``.

Mirrors blackjax/smc/ess.py ``ess``, ``log_ess`` and ``ess_solver`` for one ``(N,)`` vector of log-weights on the
device (``bjx_smc_log_ess`` / ``bjx_smc_ess_solve``, include/bjx_hip.h "SMC": fp64 sums, device scalars out).
"""
from __future__ import annotations

from typing import Callable

import torch

from .. import _lib
from .._util import check_batch, eval_logdensity, value_and_grad
from . import solver
from .base import check_particles

__all__ = ["ess", "log_ess", "ess_solver"]


def log_ess(log_weights) -> torch.Tensor:
    """blackjax/smc/ess.py ``log_ess``: ``2 logsumexp(lw) - logsumexp(2 lw)`` as a 0-d device tensor.  Entries that
    are NaN or ``-inf`` are particles of weight 0."""
    lw = check_batch(log_weights, "log_weights")
    if lw.ndim != 1 or lw.shape[0] < 1:
        raise ValueError(f"log_weights must be (n_particles,), got {tuple(lw.shape)}")
    out = torch.empty((), dtype=torch.float32, device=lw.device)
    _lib.call("bjx_smc_log_ess", _lib.current_stream(), lw.shape[0], lw.data_ptr(), out.data_ptr())
    return out


def ess(log_weights) -> torch.Tensor:
    """blackjax/smc/ess.py ``ess``."""
    return torch.exp(log_ess(log_weights))


def ess_solver(logdensity_fn: Callable, particles, target_ess, max_delta, root_solver: Callable = solver.dichotomy):
    """blackjax/smc/ess.py ``ess_solver``: the increment ``delta`` in ``[0, max_delta]`` at which the ESS of the
    log-weights ``delta * logdensity_fn(particles)`` meets ``target_ess * N``.  ``root_solver(loglikelihood,
    target_ess, max_delta)`` receives the ``(N,)`` values, not a closure over ``delta``."""
    x = check_particles(particles)
    ll, _ = eval_logdensity(value_and_grad(logdensity_fn), x)
    return root_solver(ll, target_ess, max_delta)
