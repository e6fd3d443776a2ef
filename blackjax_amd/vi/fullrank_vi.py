"""Full-rank variational inference on MI355X behind the ``blackjax.fullrank_vi`` API surface.

Mirrors blackjax/vi/fullrank_vi.py: ``FRVIState``, ``FRVIInfo``, ``init``, ``step``, ``sample``,
``generate_fullrank_logdensity`` and ``as_top_level_api``.  The approximation is ``q = N(mu, L L^T)`` with a lower
triangular ``L``; a step draws ``num_samples`` points ``mu + L eps`` from it, evaluates the target and its gradient
there, and moves ``(mu, chol_params)`` down the gradient of the Monte-Carlo estimate of ``KL(q || p)``.  With
``stl_estimator=True`` (sticking the landing, Roeder et al. 2017) the parameters inside ``log q`` carry no gradient.
Where ``meanfield_vi`` offers the samplers a diagonal metric, this fit offers the dense one:
``cholesky_factor(state)`` is ``L``, and ``L @ L.T`` is a dense ``inverse_mass_matrix`` for ``hmc`` / ``nuts``.  A
mean-field fit of a correlated target underestimates every marginal variance and has no correlations.

``chol_params`` is ``(D (D + 1) / 2,)``: the first ``D`` entries are the log-diagonal, ``L_ii = exp(chol_params[i])``,
the rest the strict lower triangle in ``torch.tril_indices(D, D, -1)`` order -- entry ``(i, j < i)`` at
``D + i (i - 1) / 2 + j``, so a row of ``L`` is contiguous.  ``init`` gives ``mu = 0`` and ``L = I``.

A step is, in this order: ``bjx_vi_fullrank_sample`` (a triangular matrix product, one launch); the user's log-density
on the ``(S, D)`` batch through ``_util.value_and_grad``; ``bjx_vi_fullrank_grad`` (under STL a batched triangular
solve ``L^T u_s = eps_s``, then the lower-triangular outer-product reduction ``mean_s w_s eps_s^T`` over the draws, the
column sums and the scalar; the noise is regenerated from the key, no ``(S, D)`` noise array exists);
``optimizer.update``; the two additions.  The launches are declared in include/bjx_hip.h under "VI".  After the
first step nothing is read back from the device: ``rng_key`` and the optimiser's step count are host values.

``position`` is one ``(D,)`` device tensor (pytrees are out of scope) and gives shape and device only.  The draws use
the key itself: ``eps = jax.random.normal(rng_key, (S, D))``, as in ``meanfield_vi``, and ``step`` draws what
``sample(rng_key, state, num_samples)`` returns.  A NaN in the target's value or gradient gives NaN outputs, as in the
reference.  Parity with a real JAX run is unpinned; the arithmetic is held against a NumPy
restatement of the reference (tests/fullrank_vi_restatement.py).
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

__all__ = ["FRVIState", "FRVIInfo", "init", "step", "sample", "kl_and_grad", "generate_fullrank_logdensity",
           "cholesky_factor", "as_top_level_api", "DRAW_TILE", "COL_BLOCK", "MAX_DIM"]

DRAW_TILE = 64  # draws per workgroup of the draw and the solve (bjx_vi_fullrank_tile())
COL_BLOCK = 64  # columns per block of the triangle (bjx_vi_fullrank_block())
MAX_DIM = 4096  # include/bjx_hip.h "VI"


class FRVIState(NamedTuple):
    """blackjax/vi/fullrank_vi.py ``FRVIState``: (D,) and (D (D + 1) / 2,) fp32 device tensors and the optimiser's
    state."""

    mu: torch.Tensor
    chol_params: torch.Tensor
    opt_state: Any


class FRVIInfo(NamedTuple):
    """blackjax/vi/fullrank_vi.py ``FRVIInfo``.  The field keeps the reference's name and, as there, holds the
    Monte-Carlo estimate of ``KL(q || p)`` that the step minimises: a 0-d device tensor."""

    elbo: torch.Tensor


def _parameters(mu, chol_params, what: str = "state"):
    mu, chol = check_batch(mu, f"{what}.mu"), check_batch(chol_params, f"{what}.chol_params")
    if mu.ndim != 1 or mu.shape[0] < 1 or chol.ndim != 1 or chol.device != mu.device:
        raise ValueError(f"{what}.mu and {what}.chol_params must be (dim,) and (dim (dim + 1) / 2,) tensors on one "
                         f"device, got {tuple(mu.shape)} on {mu.device} and {tuple(chol.shape)} on {chol.device}")
    D = mu.shape[0]
    if chol.shape[0] != D * (D + 1) // 2:
        raise ValueError(f"{what}.chol_params must have dim (dim + 1) / 2 = {D * (D + 1) // 2} entries for dim {D}, "
                         f"got {chol.shape[0]}")
    if D > MAX_DIM:
        raise ValueError(f"fullrank_vi: dimension {D} is out of range, at most {MAX_DIM} (include/bjx_hip.h, VI)")
    return mu, chol


def init(position: torch.Tensor, optimizer) -> FRVIState:
    """blackjax/vi/fullrank_vi.py ``init``: ``mu = 0``, ``chol_params = 0`` (``L = I``), the optimiser's state for
    ``(mu, chol_params)``."""
    position = _common.position(position)
    D = position.shape[0]
    if D > MAX_DIM:
        raise ValueError(f"fullrank_vi: dimension {D} is out of range, at most {MAX_DIM} (include/bjx_hip.h, VI)")
    mu = torch.zeros_like(position)
    chol = torch.zeros(D * (D + 1) // 2, dtype=position.dtype, device=position.device)
    return FRVIState(mu, chol, optimizer.init((mu, chol)))


def _draw(k0: int, k1: int, mu: torch.Tensor, chol: torch.Tensor, S: int) -> torch.Tensor:
    D = mu.shape[0]
    if _lib.load().bjx_vi_fullrank_grad_workspace_bytes(S, D) <= 0:
        raise ValueError(f"fullrank_vi: {S} draws of dimension {D} are out of range (include/bjx_hip.h, VI)")
    z = torch.empty((S, D), dtype=torch.float32, device=mu.device)
    _lib.call("bjx_vi_fullrank_sample", _lib.current_stream(), k0, k1, S, D, mu.data_ptr(), chol.data_ptr(),
              z.data_ptr())
    return z


def sample(rng_key, state: FRVIState, num_samples: int = 1) -> torch.Tensor:
    """blackjax/vi/fullrank_vi.py ``sample``: ``(num_samples, D)`` draws ``mu + L eps`` with
    ``eps = normal(rng_key, (num_samples, D))``, one launch."""
    mu, chol = _parameters(state.mu, state.chol_params)
    k0, k1 = key_words(rng_key)
    with torch.cuda.device(mu.device):
        return _draw(k0, k1, mu, chol, _common.num_samples(num_samples))


def kl_and_grad(rng_key, mu, chol_params, logp, grad, stl_estimator: bool = True):
    """The reduction of a step, ``bjx_vi_fullrank_grad``: from the target's values ``logp`` ``(S,)`` and gradients
    ``grad`` ``(S, D)`` at the draws ``sample`` makes from ``rng_key``, ``(kl, g_mu, g_chol)``: the Monte-Carlo
    estimate ``mean_s(log q(z_s) - logp_s)`` (0-d) and its gradients with respect to ``mu`` ``(D,)`` and
    ``chol_params`` ``(D (D + 1) / 2,)``.  The draws themselves are not an argument: the kernels regenerate their
    noise from the key."""
    return _common.kl_and_grad("fullrank_vi", "bjx_vi_fullrank_grad", _parameters, rng_key, mu, chol_params, logp, grad,
                               stl_estimator)


def step(rng_key, state: FRVIState, logdensity_fn: Callable, optimizer, num_samples: int = 5,
         stl_estimator: bool = True):
    """blackjax/vi/fullrank_vi.py ``step``: one stochastic gradient step on the KL estimate.
    -> ``(FRVIState, FRVIInfo)``."""
    mu, chol = _parameters(state.mu, state.chol_params)
    return _common.step(_draw, kl_and_grad, FRVIState, FRVIInfo, rng_key, mu, chol, state.opt_state, logdensity_fn,
                        optimizer, num_samples, stl_estimator)


def _unflatten_cholesky(chol_params: torch.Tensor) -> torch.Tensor:
    """blackjax/vi/fullrank_vi.py ``_unflatten_cholesky``: the ``(D, D)`` factor ``L`` of a ``(D (D + 1) / 2,)``
    parameter vector, ``exp`` of the first ``D`` entries on the diagonal.  Plain PyTorch: not on the step's path."""
    n = chol_params.shape[0]
    D = (math.isqrt(8 * n + 1) - 1) // 2
    if chol_params.ndim != 1 or D < 1 or D * (D + 1) // 2 != n:
        raise ValueError(f"chol_params must be (dim (dim + 1) / 2,), got {tuple(chol_params.shape)}")
    L = torch.diag(torch.exp(chol_params[:D]))
    rows, cols = torch.tril_indices(D, D, -1, device=chol_params.device)
    L[rows, cols] = chol_params[D:]
    return L


def cholesky_factor(state: FRVIState) -> torch.Tensor:
    """The lower triangular ``L`` of ``q = N(mu, L L^T)``, ``(D, D)``.  ``L @ L.T`` is the fitted covariance: what a
    dense ``inverse_mass_matrix`` of ``hmc`` / ``nuts`` takes."""
    return _unflatten_cholesky(state.chol_params)


def generate_fullrank_logdensity(mu, cov) -> Callable:
    """blackjax/vi/fullrank_vi.py ``generate_fullrank_logdensity``: the batched log-density of ``N(mu, cov)``,
    ``z (S, D) -> (S,)``.  Plain PyTorch: not on the step's path."""
    L = torch.linalg.cholesky(cov)
    D = mu.shape[0]
    const = 0.5 * D * math.log(2.0 * math.pi) + torch.log(torch.diagonal(L)).sum()

    def fullrank_logdensity(position):
        u = torch.linalg.solve_triangular(L, (position - mu).unsqueeze(-1), upper=False).squeeze(-1)
        return -0.5 * (u * u).sum(-1) - const

    return fullrank_logdensity


def as_top_level_api(logdensity_fn: Callable, optimizer, num_samples: int = 100) -> VIAlgorithm:
    """blackjax/vi/fullrank_vi.py ``as_top_level_api``: ``init(position)``, ``step(rng_key, state)``,
    ``sample(rng_key, state, num_samples=1)``."""
    return _common.as_top_level_api(init, step, sample, logdensity_fn, optimizer, num_samples)
