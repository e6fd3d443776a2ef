"""Batched elliptical slice sampler on MI355X behind the ``blackjax.elliptical_slice`` API surface.

Mirrors blackjax/mcmc/elliptical_slice.py: ``EllipSliceState``, ``EllipSliceInfo``, ``init``, ``build_kernel`` and
``as_top_level_api``.  The model is a Gaussian prior ``N(mean, cov)`` times an arbitrary likelihood; the callable is
the log-LIKELIHOOD over the batch.  It needs no gradient, has no step size and no warm-up, and never rejects: every
transition shrinks an angle bracket on the ellipse through the current position and a fresh prior draw until the
proposal lies on the slice.

The chain axis is native; chain ``i`` of ``step(rng_key, state)`` reproduces the reference's single-chain
``step(jax.random.split(rng_key, N)[chain_offset + i], state_i)``.  ``mean`` is ``(D,)`` or a Python scalar;
``cov`` is ``(D,)`` (diagonal) or ``(D, D)`` (dense, factorised once in fp64), shared by all chains -- a 2-d ``cov`` is
always dense, so there is no ``N == D`` ambiguity.  Like every RNG-dependent part of the package, parity with a real
JAX run is unpinned; the arithmetic is held against a NumPy restatement of the reference
(tests/elliptical_slice_restatement.py).

The callable is called on a detached ``(N, D)`` tensor under ``torch.no_grad()`` and may return ``logp (N,)`` or a
``(logp, grad)`` pair, of which only ``logp`` is used.  It is never traced and never differentiated.

The arithmetic runs in libbjxhip (include/bjx_hip.h, "elliptical slice"); this module sequences
begin (one launch; the dense prior adds a noise launch and the MFMA GEMM) -> user callable ->
{ shrink (one launch) -> read the live count -> user callable } until no chain is live.  Chains need different
numbers of rounds; the callable sees all ``N`` rows every round and the rows of finished chains are ignored.

The one deliberate difference from the reference: its ``while_loop`` has no cap, so a likelihood that is ``-inf``
everywhere never ends.  Here a transition that still has live chains after ``max_subiter`` likelihood evaluations
raises ``RuntimeError``.
"""
from __future__ import annotations

from typing import Callable, NamedTuple

import torch

from . import _lib
from ._util import check_batch
from .base import SamplingAlgorithm
from .random import key_spec

__all__ = ["EllipSliceState", "EllipSliceInfo", "init", "build_kernel", "as_top_level_api"]


class EllipSliceState(NamedTuple):
    """blackjax/mcmc/elliptical_slice.py ``EllipSliceState``, batched: (N, D), (N,).  ``logdensity`` is the
    log-likelihood, as in the reference."""

    position: torch.Tensor
    logdensity: torch.Tensor


class EllipSliceInfo(NamedTuple):
    """blackjax/mcmc/elliptical_slice.py ``EllipSliceInfo``, batched: (N, D) float32, (N,) float32, (N,) int32."""

    momentum: torch.Tensor
    theta: torch.Tensor
    subiter: torch.Tensor


def _loglikelihood(logdensity_fn: Callable, q: torch.Tensor) -> torch.Tensor:
    """The callable's log-likelihood at ``q`` as contiguous fp32 ``(N,)``; the gradient of a pair is dropped."""
    with torch.no_grad():
        out = logdensity_fn(q.detach())
    if isinstance(out, (tuple, list)):
        out = out[0]
    if out.shape != q.shape[:1]:
        raise ValueError(f"logdensity_fn must return logp of shape {tuple(q.shape[:1])}, got {tuple(out.shape)}")
    if out.dtype != torch.float32:
        out = out.float()
    return out.detach().contiguous()


def init(position: torch.Tensor, logdensity_fn: Callable) -> EllipSliceState:
    """blackjax/mcmc/elliptical_slice.py ``init``: the log-likelihood at the initial positions."""
    position = check_batch(position, "position")
    if position.ndim != 2:
        raise ValueError(f"position must be (n_chains, dim), got {tuple(position.shape)}")
    return EllipSliceState(position, _loglikelihood(logdensity_fn, position))


class _Prior(NamedTuple):
    mean: torch.Tensor  # (D,)
    cov_diag: torch.Tensor | None  # (D,) [diag]
    chol_t: torch.Tensor | None  # (D, D) [dense]: L^T row-major, L = cholesky(cov) in fp64 rounded once


def _check_prior(mean, cov, dim: int):
    """Shapes of ``mean`` / ``cov`` against ``dim`` (host-side: no device is touched)."""
    if not isinstance(mean, (int, float)):
        mean = torch.as_tensor(mean)
        if mean.ndim == 2:
            raise NotImplementedError("a per-chain mean is not supported: mean must be (dim,) or a scalar")
        if mean.ndim != 1 and mean.ndim != 0:
            raise ValueError(f"The mean has the wrong number of dimensions: expected 0 or 1, got {mean.ndim}.")
        if mean.ndim == 1 and mean.shape[0] != dim:
            raise ValueError(f"mean has {mean.shape[0]} entries, position has {dim}")
    cov = torch.as_tensor(cov)
    if cov.ndim == 1:
        if cov.shape[0] != dim:
            raise ValueError(f"cov has {cov.shape[0]} entries, position has {dim}")
    elif cov.ndim == 2:
        if cov.shape[0] != cov.shape[1]:
            raise ValueError(f"a 2-d cov is a dense matrix and must be square, got {tuple(cov.shape)} "
                             "(per-chain diagonals are not supported)")
        if cov.shape[0] != dim:
            raise ValueError(f"cov is {tuple(cov.shape)}, position has {dim} dims")
    elif cov.ndim == 3:
        raise NotImplementedError("a per-chain cov is not supported: cov must be (dim,) or (dim, dim)")
    else:
        raise ValueError(f"The covariance has the wrong number of dimensions: expected 1 or 2, got {cov.ndim}.")
    return mean, cov


def _prepare_prior(mean, cov, dim: int, device) -> _Prior:
    mean, cov = _check_prior(mean, cov, dim)
    if isinstance(mean, (int, float)) or mean.ndim == 0:
        mean_t = torch.full((dim,), float(mean), dtype=torch.float32, device=device)
    else:
        mean_t = mean.to(device=device, dtype=torch.float32).contiguous()
    cov = cov.to(device=device, dtype=torch.float32)
    if cov.ndim == 1:
        return _Prior(mean_t, cov.contiguous(), None)
    L = torch.linalg.cholesky(cov.double())  # as metrics._dense_metric: fp64, rounded once
    return _Prior(mean_t, None, L.float().t().contiguous())


def build_kernel(cov_matrix, mean):
    """blackjax/mcmc/elliptical_slice.py ``build_kernel``.  ``cov_matrix``: ``(D,)`` or ``(D, D)``; ``mean``: ``(D,)`` or
    a scalar.  The prior is prepared (moved to the device, factorised when dense) at the first transition of each
    (dim, device) and kept."""
    if not isinstance(mean, (int, float)) and torch.as_tensor(mean).ndim == 2:
        raise NotImplementedError("a per-chain mean is not supported: mean must be (dim,) or a scalar")
    nd = torch.as_tensor(cov_matrix).ndim
    if nd == 3:
        raise NotImplementedError("a per-chain cov is not supported: cov must be (dim,) or (dim, dim)")
    if nd not in (1, 2):
        raise ValueError(f"The covariance has the wrong number of dimensions: expected 1 or 2, got {nd}.")
    priors: dict = {}

    def kernel(rng_key, state: EllipSliceState, logdensity_fn: Callable, *, chain_offset: int = 0,
               max_subiter: int = 1024):
        if not isinstance(state.position, torch.Tensor) or state.position.ndim != 2:
            raise ValueError(f"state.position must be (n_chains, dim), got {tuple(getattr(state.position, 'shape', ()))}")
        N, D = state.position.shape
        prior = priors.get((D, state.position.device))
        if prior is None:
            _check_prior(mean, cov_matrix, D)  # shape errors come before the device check
        q0 = check_batch(state.position, "state.position")
        logp0 = check_batch(state.logdensity, "state.logdensity")
        if logp0.shape != (N,):
            raise ValueError(f"state.logdensity must be ({N},), got {tuple(logp0.shape)}")
        max_subiter = int(max_subiter)
        if max_subiter < 1:
            raise ValueError(f"max_subiter must be at least 1, got {max_subiter}")
        dev = q0.device
        if prior is None:
            prior = priors[(D, dev)] = _prepare_prior(mean, cov_matrix, D, dev)
        k0, k1, fold = key_spec(rng_key)
        off = int(chain_offset)
        stream = _lib.current_stream()

        nu, q_prop, momentum = torch.empty_like(q0), torch.empty_like(q0), torch.empty_like(q0)
        logy, theta, theta_min, theta_max = (torch.empty_like(logp0) for _ in range(4))
        logp_new, theta_new = torch.empty_like(logp0), torch.empty_like(logp0)
        subiter = torch.empty(N, dtype=torch.int32, device=dev)
        subiter_new = torch.empty(N, dtype=torch.int32, device=dev)
        done = torch.empty(N, dtype=torch.uint8, device=dev)
        new = EllipSliceState(q_prop, logp_new), EllipSliceInfo(momentum, theta_new, subiter_new)
        if N == 0:
            return new

        nu_lin = None
        if prior.chol_t is not None:
            noise, nu_lin = torch.empty_like(q0), torch.empty_like(q0)
            _lib.call("bjx_ess_noise", stream, k0, k1, off, fold, N, D, noise.data_ptr())
            _lib.call("bjx_dense_matmul", stream, N, D, noise.data_ptr(), prior.chol_t.data_ptr(), nu_lin.data_ptr())
        _lib.call("bjx_ess_begin", stream, k0, k1, off, fold, N, D, prior.mean.data_ptr(), _lib.ptr(prior.cov_diag),
                  _lib.ptr(nu_lin), q0.data_ptr(), logp0.data_ptr(), nu.data_ptr(), q_prop.data_ptr(),
                  logy.data_ptr(), theta.data_ptr(), theta_min.data_ptr(), theta_max.data_ptr(),
                  subiter.data_ptr(), done.data_ptr())
        # one zeroed live counter per round: a single fill per transition instead of one per launch
        n_live = torch.zeros(max_subiter, dtype=torch.int32, device=dev)
        for it in range(max_subiter):
            logp_prop = _loglikelihood(logdensity_fn, q_prop)  # may be a new tensor every round
            _lib.call("bjx_ess_shrink", stream, k0, k1, off, fold, N, D, prior.mean.data_ptr(), q0.data_ptr(),
                      nu.data_ptr(), logp_prop.data_ptr(), logy.data_ptr(), theta.data_ptr(), theta_min.data_ptr(),
                      theta_max.data_ptr(), subiter.data_ptr(), done.data_ptr(), q_prop.data_ptr(),
                      logp_new.data_ptr(), theta_new.data_ptr(), subiter_new.data_ptr(), momentum.data_ptr(),
                      n_live[it:].data_ptr())
            live = int(n_live[it])  # blocking 4-byte read
            if live == 0:
                return new
        raise RuntimeError(
            f"elliptical_slice: {live} of {N} chains were still shrinking their bracket after max_subiter="
            f"{max_subiter} likelihood evaluations (a likelihood that is -inf almost everywhere, or a state whose "
            "logdensity is not the likelihood of its position?)")

    return kernel


def as_top_level_api(loglikelihood_fn: Callable, *, mean, cov, chain_offset: int = 0,
                     max_subiter: int = 1024) -> SamplingAlgorithm:
    """blackjax/mcmc/elliptical_slice.py ``as_top_level_api``: ``init(position)``, ``step(rng_key, state)``."""
    kernel = build_kernel(cov, mean)

    def init_fn(position, rng_key=None):
        del rng_key
        return init(position, loglikelihood_fn)

    def step_fn(rng_key, state):
        return kernel(rng_key, state, loglikelihood_fn, chain_offset=chain_offset, max_subiter=max_subiter)

    return SamplingAlgorithm(init_fn, step_fn)
