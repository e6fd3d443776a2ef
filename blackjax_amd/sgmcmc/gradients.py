"""Minibatch estimators of the log-density and its gradient, behind ``blackjax.sgmcmc.gradients``.

Mirrors blackjax/sgmcmc/gradients.py: ``logdensity_estimator``, ``grad_estimator`` and ``control_variates``, batched
over the chain axis.  Plain PyTorch: the cost here is the user's model, and the minibatch changes every step, so
nothing is traced and nothing is cached on the minibatch.  The helpers work on tensors of any device; only the
samplers insist on device tensors.

* ``logprior_fn``: ``(N, D) -> (N,)``.
* ``loglikelihood_fn``: ``((N, D), minibatch) -> (N, B)``, the log-likelihood of every datum of the minibatch.
  ``minibatch`` is whatever the caller's functions understand; it is handed on untouched.
"""
from __future__ import annotations

from typing import Callable

import torch

__all__ = ["logdensity_estimator", "grad_estimator", "control_variates"]


def logdensity_estimator(logprior_fn: Callable, loglikelihood_fn: Callable, data_size: int) -> Callable:
    """blackjax/sgmcmc/gradients.py ``logdensity_estimator``:
    ``logprior_fn(position) + data_size * mean over the minibatch of loglikelihood_fn(position, minibatch)``."""

    def logdensity_estimator_fn(position, minibatch):
        return logprior_fn(position) + data_size * loglikelihood_fn(position, minibatch).mean(-1)

    return logdensity_estimator_fn


def grad_estimator(logprior_fn: Callable, loglikelihood_fn: Callable, data_size: int) -> Callable:
    """blackjax/sgmcmc/gradients.py ``grad_estimator``: the per-chain gradient of ``logdensity_estimator``, taken with
    ``torch.autograd.grad`` of the sum over chains (chains are independent, so that IS the per-chain gradient)."""
    logdensity_estimator_fn = logdensity_estimator(logprior_fn, loglikelihood_fn, data_size)

    def grad_estimator_fn(position, minibatch):
        q = position.detach().requires_grad_(True)
        with torch.enable_grad():
            (g,) = torch.autograd.grad(logdensity_estimator_fn(q, minibatch).sum(), q)
        return g

    return grad_estimator_fn


def control_variates(logdensity_grad_estimator: Callable, centering_position, data) -> Callable:
    """blackjax/sgmcmc/gradients.py ``control_variates``: the estimator's full-data gradient at the centring position,
    evaluated once here, plus the minibatch difference between the position and the centre.  ``centering_position``
    is ``(D,)`` (one centre for every chain) or ``(N, D)``."""
    centre = centering_position[None] if centering_position.ndim == 1 else centering_position
    cv_grad_value = logdensity_grad_estimator(centre, data)

    def cv_grad_estimator_fn(position, minibatch):
        return (cv_grad_value + logdensity_grad_estimator(position, minibatch)
                - logdensity_grad_estimator(centre, minibatch))

    return cv_grad_estimator_fn
