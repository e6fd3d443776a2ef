"""Mean-field variational inference on MI355X behind the ``blackjax.meanfield_vi`` API surface.

Mirrors blackjax/vi/meanfield_vi.py: ``MFVIState``, ``MFVIInfo``, ``init``, ``step``, ``sample``,
``generate_meanfield_logdensity`` and ``as_top_level_api``.  The approximation is ``q = N(mu, exp(rho)^2)`` with a
diagonal covariance; a step draws ``num_samples`` points from it by reparameterisation, evaluates the target and its
gradient there, and moves ``(mu, rho)`` down the gradient of the Monte-Carlo estimate of ``KL(q || p)``.  With
``stl_estimator=True`` (sticking the landing, Roeder et al. 2017) the parameters inside ``log q`` carry no gradient,
which removes the estimator's variance at the optimum.  Its typical use here is a cheap approximate posterior, or a
starting point and a diagonal metric (``torch.exp(2 * state.rho)``) for the samplers of this package.

The ``num_samples`` draws are an ``(S, D)`` row batch.  A step is, in this order: ``bjx_vi_meanfield_sample`` (one
launch); the user's log-density on the batch through ``_util.value_and_grad`` (a plain PyTorch function is traced once
into one HIP value-and-gradient kernel, as for ``mala``); ``bjx_vi_meanfield_grad`` (the ``(S, D)`` gradients reduced
to two ``(D,)`` gradients and the KL estimate, the noise regenerated from the key: no ``(S, D)`` noise array exists);
``optimizer.update`` (one launch per parameter for ``blackjax_amd.optim.adam`` / ``sgd``); the two additions.  The
launches are declared in include/bjx_hip.h under "VI".  After the first step nothing is read back from the device:
``rng_key`` and the optimiser's step count are host values.

``position`` is one ``(D,)`` device tensor (pytrees are out of scope) and gives shape and device only.  The draws use
the key itself: element ``(s, d)`` is ``jax.random.normal(rng_key, (S, D))[s, d]``, and ``step`` draws what
``sample(rng_key, state, num_samples)`` returns.  A NaN in the target's value or gradient gives NaN outputs, as in the
reference.  Like every RNG-dependent part of the package, parity with a real JAX run is unpinned;
the arithmetic is held against a NumPy restatement of the reference (tests/meanfield_vi_restatement.py).
"""
from __future__ import annotations

import math
from typing import Any, Callable, NamedTuple

import torch

from .. import _lib
from .._util import check_batch
from ..base import VIAlgorithm
from ..random import key_words
from . import _common

__all__ = ["MFVIState", "MFVIInfo", "init", "step", "sample", "kl_and_grad", "generate_meanfield_logdensity",
           "as_top_level_api", "GRAD_TILE"]

GRAD_TILE = 64  # rows per workgroup of the reduction (bjx_vi_meanfield_tile())


class MFVIState(NamedTuple):
    """blackjax/vi/meanfield_vi.py ``MFVIState``: (D,), (D,) fp32 device tensors and the optimiser's state."""

    mu: torch.Tensor
    rho: torch.Tensor
    opt_state: Any


class MFVIInfo(NamedTuple):
    """blackjax/vi/meanfield_vi.py ``MFVIInfo``.  The field keeps the reference's name and, as there, holds the
    Monte-Carlo estimate of ``KL(q || p)`` that the step minimises: a 0-d device tensor."""

    elbo: torch.Tensor


def _parameters(mu, rho, what: str = "state"):
    mu, rho = check_batch(mu, f"{what}.mu"), check_batch(rho, f"{what}.rho")
    if mu.ndim != 1 or mu.shape[0] < 1 or rho.shape != mu.shape or rho.device != mu.device:
        raise ValueError(f"{what}.mu and {what}.rho must be (dim,) tensors on one device, got {tuple(mu.shape)} on "
                         f"{mu.device} and {tuple(rho.shape)} on {rho.device}")
    return mu, rho


def init(position: torch.Tensor, optimizer) -> MFVIState:
    """blackjax/vi/meanfield_vi.py ``init``: ``mu = 0``, ``rho = -2``, the optimiser's state for ``(mu, rho)``."""
    position = _common.position(position)
    mu = torch.zeros_like(position)
    rho = torch.full_like(position, -2.0)
    return MFVIState(mu, rho, optimizer.init((mu, rho)))


def _draw(k0: int, k1: int, mu: torch.Tensor, rho: torch.Tensor, S: int) -> torch.Tensor:
    z = torch.empty((S, mu.shape[0]), dtype=torch.float32, device=mu.device)
    _lib.call("bjx_vi_meanfield_sample", _lib.current_stream(), k0, k1, S, mu.shape[0], mu.data_ptr(), rho.data_ptr(),
              z.data_ptr())
    return z


def sample(rng_key, state: MFVIState, num_samples: int = 1) -> torch.Tensor:
    """blackjax/vi/meanfield_vi.py ``sample``: ``(num_samples, D)`` draws ``mu + exp(rho) * eps`` with
    ``eps = normal(rng_key, (num_samples, D))``, one launch."""
    mu, rho = _parameters(state.mu, state.rho)
    k0, k1 = key_words(rng_key)
    with torch.cuda.device(mu.device):
        return _draw(k0, k1, mu, rho, _common.num_samples(num_samples))


def kl_and_grad(rng_key, mu, rho, logp, grad, stl_estimator: bool = True):
    """The reduction of a step, ``bjx_vi_meanfield_grad``: from the target's values ``logp`` ``(S,)`` and gradients
    ``grad`` ``(S, D)`` at the draws ``sample`` makes from ``rng_key``, ``(kl, g_mu, g_rho)``: the Monte-Carlo
    estimate ``mean_s(log q(z_s) - logp_s)`` (0-d) and its gradients with respect to ``mu`` and ``rho`` (``(D,)``).
    The draws themselves are not an argument: the kernel regenerates their noise from the key."""
    return _common.kl_and_grad("meanfield_vi", "bjx_vi_meanfield_grad", _parameters, rng_key, mu, rho, logp, grad,
                               stl_estimator)


def step(rng_key, state: MFVIState, logdensity_fn: Callable, optimizer, num_samples: int = 5,
         stl_estimator: bool = True):
    """blackjax/vi/meanfield_vi.py ``step``: one stochastic gradient step on the KL estimate.
    -> ``(MFVIState, MFVIInfo)``."""
    mu, rho = _parameters(state.mu, state.rho)
    return _common.step(_draw, kl_and_grad, MFVIState, MFVIInfo, rng_key, mu, rho, state.opt_state, logdensity_fn,
                        optimizer, num_samples, stl_estimator)


def generate_meanfield_logdensity(mu, rho) -> Callable:
    """blackjax/vi/meanfield_vi.py ``generate_meanfield_logdensity``: the batched log-density of the approximation,
    ``z (S, D) -> (S,)``, the sum over the dimensions of the normal log-pdfs.  Plain PyTorch: not on the step's path."""
    sigma = torch.exp(rho)
    const = 0.5 * math.log(2.0 * math.pi)

    def meanfield_logdensity(position):
        u = (position - mu) / sigma
        return (-0.5 * u * u - rho - const).sum(-1)

    return meanfield_logdensity


def as_top_level_api(logdensity_fn: Callable, optimizer, num_samples: int = 100) -> VIAlgorithm:
    """blackjax/vi/meanfield_vi.py ``as_top_level_api``: ``init(position)``, ``step(rng_key, state)``,
    ``sample(rng_key, state, num_samples=1)``."""
    return _common.as_top_level_api(init, step, sample, logdensity_fn, optimizer, num_samples)
