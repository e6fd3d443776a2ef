"""Batched marginal latent-Gaussian sampler on MI355X behind the ``blackjax.mgrad_gaussian`` API surface.

Mirrors blackjax/mcmc/marginal_latent_gaussian.py: ``MarginalState``, ``MarginalInfo``, ``CovarianceSVD``,
``svd_from_covariance``, ``generate_mean_shifted_logprob``, ``init``, ``build_kernel`` and ``as_top_level_api``.  It
is the auxiliary marginal sampler of Titsias & Papaspiliopoulos (2018) for a Gaussian prior ``N(mean, C)`` times an
arbitrary likelihood; the callable is the log-LIKELIHOOD over the batch.  One value-and-gradient call per transition,
a fixed launch sequence and no host read; the proposal is preconditioned by the prior covariance
``C = U diag(Gamma) U^T``, so it mixes where ``mala`` needs a tiny step.  There is no warm-up; the reference has none.

The chain axis is native; chain ``i`` of ``step(rng_key, state)`` reproduces the reference's single-chain
``step(jax.random.split(rng_key, N)[chain_offset + i], state_i)``.  Like every RNG-dependent part of the package,
parity with a real JAX run is unpinned; the arithmetic is held against a NumPy restatement of
the reference (tests/mgrad_gaussian_restatement.py).

The arithmetic runs in libbjxhip (include/bjx_hip.h, "marginal latent Gaussian"); this module sequences, for a dense
prior,

    propose -> bjx_dense_matmul(t, U_t) = y -> user value-and-grad [-> shift]
            -> bjx_dense_matmul_bt(y, U, U_t) = U_y -> bjx_dense_matmul_bt(g_y, U, U_t) = U_grad_y -> finish

Deliberate differences from the reference:

1. A NaN ``log_ratio`` goes through ``safe_energy_diff``: the proposal is rejected, as in the reference, and
   ``acceptance_rate`` is 0 instead of NaN (the package's rule for ``mala``).
2. ``step_size`` may be a per-chain ``(N,)`` tensor.
3. A 1-d ``covariance`` ``(D,)`` is a diagonal prior: ``U = I``, ``Gamma = covariance`` and no GEMM is launched;
   ``state.U_x`` IS ``state.position`` and ``state.U_grad_x`` IS ``state.logdensity_grad`` (the same tensors).  A 2-d
   covariance is always dense; a 3-d one (per-chain priors) raises ``NotImplementedError``.
4. ``cov_svd`` together with ``mean`` and without ``covariance`` is accepted: ``shift = U ((U_t mean) / Gamma)``.
   The factorisation (``torch.linalg.eigh`` on the CPU, eigenvalues descending to match an SVD), ``shift`` and the
   fp32 copies of ``U`` / ``U_t`` are computed once on the host in fp64 and rounded once.  Non-positive eigenvalues
   raise ``ValueError``.
"""
from __future__ import annotations

from typing import Callable, NamedTuple

import torch

from . import _lib
from ._util import check_batch, eval_logdensity, step_size_args, value_and_grad
from .base import SamplingAlgorithm
from .random import key_spec

__all__ = ["MarginalState", "MarginalInfo", "CovarianceSVD", "svd_from_covariance", "generate_mean_shifted_logprob",
           "init", "build_kernel", "as_top_level_api"]


class MarginalState(NamedTuple):
    """blackjax/mcmc/marginal_latent_gaussian.py ``MarginalState``, batched: (N, D), (N,), (N, D), (N, D), (N, D).
    ``logdensity`` is the (mean-shifted) log-likelihood, as in the reference."""

    position: torch.Tensor
    logdensity: torch.Tensor
    logdensity_grad: torch.Tensor
    U_x: torch.Tensor
    U_grad_x: torch.Tensor


class MarginalInfo(NamedTuple):
    """blackjax/mcmc/marginal_latent_gaussian.py ``MarginalInfo``, batched: (N,) float32, (N,) bool, the proposal."""

    acceptance_rate: torch.Tensor
    is_accepted: torch.Tensor
    proposal: MarginalState


class CovarianceSVD(NamedTuple):
    """blackjax/mcmc/marginal_latent_gaussian.py ``CovarianceSVD``: ``C = U diag(Gamma) U_t``, fp32, row-major.  A
    diagonal prior has ``U = U_t = None`` and ``Gamma`` the variances."""

    U: torch.Tensor | None
    Gamma: torch.Tensor
    U_t: torch.Tensor | None


def _check_covariance(covariance) -> torch.Tensor:
    """``covariance`` as a tensor of 1 or 2 dimensions (host-side: no device is touched)."""
    cov = torch.as_tensor(covariance)
    if cov.ndim == 3:
        raise NotImplementedError("a per-chain covariance is not supported: covariance must be (dim,) or (dim, dim)")
    if cov.ndim not in (1, 2):
        raise ValueError(f"The covariance has the wrong number of dimensions: expected 1 or 2, got {cov.ndim}.")
    if cov.ndim == 2 and cov.shape[0] != cov.shape[1]:
        raise ValueError(f"a 2-d covariance is a dense matrix and must be square, got {tuple(cov.shape)} "
                         "(per-chain diagonals are not supported)")
    return cov


def svd_from_covariance(covariance) -> CovarianceSVD:
    """blackjax/mcmc/marginal_latent_gaussian.py ``svd_from_covariance``.  ``(D, D)``: the symmetric eigendecomposition
    in fp64 on the host, eigenvalues descending, rounded once to fp32 and returned on ``covariance``'s device
    (``U_t`` is the exact transpose of ``U``).  ``(D,)``: a diagonal prior, ``CovarianceSVD(None, covariance, None)``."""
    cov = _check_covariance(covariance)
    if cov.ndim == 1:
        gamma = cov.detach().to(torch.float32).contiguous()
        if not bool((gamma.cpu() > 0).all()):
            raise ValueError("the covariance is not positive definite: a variance is not positive")
        return CovarianceSVD(None, gamma, None)
    c64 = cov.detach().to(device="cpu", dtype=torch.float64)
    w, v = torch.linalg.eigh(0.5 * (c64 + c64.t()))  # ascending
    w, v = w.flip(0), v.flip(1)
    if not bool((w > 0).all()):
        raise ValueError(f"the covariance is not positive definite: its smallest eigenvalue is {float(w[-1])}")
    U = v.to(torch.float32).contiguous()
    return CovarianceSVD(U.to(cov.device), w.to(torch.float32).contiguous().to(cov.device),
                         U.t().contiguous().to(cov.device))


def _check_mean(mean, dim: int | None):
    if mean is None or isinstance(mean, (int, float)):
        return mean
    mean = torch.as_tensor(mean)
    if mean.ndim == 2:
        raise NotImplementedError("a per-chain mean is not supported: mean must be (dim,) or a scalar")
    if mean.ndim not in (0, 1):
        raise ValueError(f"The mean has the wrong number of dimensions: expected 0 or 1, got {mean.ndim}.")
    if mean.ndim == 1 and dim is not None and mean.shape[0] != dim:
        raise ValueError(f"mean has {mean.shape[0]} entries, the covariance has {dim}")
    return mean


def _check_svd(cov_svd: CovarianceSVD) -> int:
    """Shapes of a factorisation (host-side); returns the dimension."""
    U, gamma, U_t = cov_svd
    if not isinstance(gamma, torch.Tensor) or gamma.ndim != 1:
        raise ValueError("cov_svd.Gamma must be a (dim,) tensor")
    D = int(gamma.shape[0])
    if (U is None) != (U_t is None):
        raise ValueError("cov_svd.U and cov_svd.U_t are given together (dense prior) or both None (diagonal prior)")
    if U is not None and (tuple(U.shape) != (D, D) or tuple(U_t.shape) != (D, D)):
        raise ValueError(f"cov_svd.U and cov_svd.U_t must be ({D}, {D}), got {tuple(U.shape)} and {tuple(U_t.shape)}")
    return D


def _shift(cov_svd: CovarianceSVD, mean) -> torch.Tensor:
    """``C^-1 mean = U ((U_t mean) / Gamma)`` from the fp32 factor, in fp64 on the host, rounded once."""
    U, gamma, U_t = cov_svd
    D = int(gamma.shape[0])
    g64 = gamma.detach().to(device="cpu", dtype=torch.float64)
    if isinstance(mean, (int, float)) or mean.ndim == 0:
        m64 = torch.full((D,), float(mean), dtype=torch.float64)
    else:
        m64 = mean.detach().to(device="cpu", dtype=torch.float64)
    if U is None:
        return (m64 / g64).to(torch.float32)
    U64 = U.detach().to(device="cpu", dtype=torch.float64)
    Ut64 = U_t.detach().to(device="cpu", dtype=torch.float64)
    return (U64 @ ((Ut64 @ m64) / g64)).to(torch.float32)


class _MeanShifted:
    """``x -> logdensity_fn(x) + dot(x, shift)`` with its gradient ``g + shift`` (one launch after the callable's own)."""

    _bjx_value_and_grad = True

    def __init__(self, logdensity_fn: Callable, shift: torch.Tensor):
        self.logdensity_fn = logdensity_fn
        self.shift = shift.detach().to(torch.float32).contiguous()
        self._on: dict = {}

    def __call__(self, q: torch.Tensor):
        if q.ndim != 2 or q.shape[1] != self.shift.shape[0]:
            raise ValueError(f"position must be (n_chains, {self.shift.shape[0]}), got {tuple(q.shape)}")
        q = check_batch(q, "position")
        shift = self._on.get(q.device)
        if shift is None:
            shift = self._on[q.device] = self.shift.to(q.device)
        logp, g = eval_logdensity(value_and_grad(self.logdensity_fn), q)
        N, D = q.shape
        logp_s, g_s = torch.empty_like(logp), torch.empty_like(g)
        _lib.call("bjx_mgrad_shift", _lib.current_stream(), N, D, shift.data_ptr(), q.data_ptr(), logp.data_ptr(),
                  g.data_ptr(), logp_s.data_ptr(), g_s.data_ptr())
        return logp_s, g_s


def generate_mean_shifted_logprob(logdensity_fn: Callable, mean, covariance) -> Callable:
    """blackjax/mcmc/marginal_latent_gaussian.py ``generate_mean_shifted_logprob``: the log-likelihood to run on the
    zero-mean prior, ``x -> logdensity_fn(x) + dot(x, C^-1 mean)``, as a ``(logp, grad)`` callable.  ``covariance``
    may be a ``CovarianceSVD``."""
    if isinstance(covariance, CovarianceSVD):
        cov_svd = covariance
    else:
        cov_svd = svd_from_covariance(covariance)
    D = _check_svd(cov_svd)
    return _MeanShifted(logdensity_fn, _shift(cov_svd, _check_mean(mean, D)))


def _rotate(a: torch.Tensor, U: torch.Tensor, U_t: torch.Tensor) -> torch.Tensor:
    """Rows of ``a`` into the eigenbasis: ``a @ U`` (row i is ``U_t a_i``)."""
    N, D = a.shape
    out = torch.empty_like(a)
    _lib.call("bjx_dense_matmul_bt", _lib.current_stream(), N, D, a.data_ptr(), U.data_ptr(), U_t.data_ptr(),
              out.data_ptr())
    return out


def _on_device(t: torch.Tensor, device) -> torch.Tensor:
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def init(position: torch.Tensor, logdensity_fn: Callable, U_t) -> MarginalState:
    """blackjax/mcmc/marginal_latent_gaussian.py ``init``: the log-likelihood and its gradient at the initial
    positions and their images in the prior's eigenbasis.  ``U_t = None``: a diagonal prior, the images are the
    position and the gradient themselves."""
    if isinstance(position, torch.Tensor) and position.ndim != 2:
        raise ValueError(f"position must be (n_chains, dim), got {tuple(position.shape)}")
    if U_t is not None and isinstance(position, torch.Tensor) and tuple(U_t.shape) != (position.shape[1],) * 2:
        raise ValueError(f"U_t is {tuple(U_t.shape)}, position has {position.shape[1]} dims")
    position = check_batch(position, "position")
    logp, grad = eval_logdensity(value_and_grad(logdensity_fn), position)
    if U_t is None:
        return MarginalState(position, logp, grad, position, grad)
    U_t = _on_device(U_t, position.device)
    U = U_t.t().contiguous()
    return MarginalState(position, logp, grad, _rotate(position, U, U_t), _rotate(grad, U, U_t))


def build_kernel(cov_svd: CovarianceSVD):
    """blackjax/mcmc/marginal_latent_gaussian.py ``build_kernel``.  The factor is moved to the device at the first
    transition of each (dim, device) and kept."""
    D_prior = _check_svd(cov_svd)
    dense = cov_svd.U is not None
    prepared: dict = {}

    def kernel(rng_key, state: MarginalState, logdensity_fn: Callable, delta, *, chain_offset: int = 0):
        if not isinstance(state.position, torch.Tensor) or state.position.ndim != 2:
            raise ValueError(f"state.position must be (n_chains, dim), got {tuple(getattr(state.position, 'shape', ()))}")
        N, D = state.position.shape
        if D != D_prior:
            raise ValueError(f"the prior has {D_prior} dims, state.position has {D}")  # before the device check
        x = check_batch(state.position, "state.position")
        logp_x = check_batch(state.logdensity, "state.logdensity")
        g_x = check_batch(state.logdensity_grad, "state.logdensity_grad")
        if logp_x.shape != (N,):
            raise ValueError(f"state.logdensity must be ({N},), got {tuple(logp_x.shape)}")
        dev = x.device
        if dense:
            U_x = check_batch(state.U_x, "state.U_x")
            U_grad_x = check_batch(state.U_grad_x, "state.U_grad_x")
        else:
            U_x, U_grad_x = x, g_x
        prior = prepared.get((D, dev))
        if prior is None:
            prior = prepared[(D, dev)] = CovarianceSVD(*(None if t is None else _on_device(t, dev) for t in cov_svd))
        U, gamma, U_t = prior
        k0, k1, fold = key_spec(rng_key)
        vg = value_and_grad(logdensity_fn)
        dlt, dlt_pc = step_size_args(delta, N, dev)
        off = int(chain_offset)
        stream = _lib.current_stream()

        t = torch.empty_like(x)
        _lib.call("bjx_mgrad_propose", stream, k0, k1, off, fold, N, D, dlt, _lib.ptr(dlt_pc), gamma.data_ptr(),
                  U_x.data_ptr(), U_grad_x.data_ptr(), t.data_ptr())
        if dense:
            y = torch.empty_like(x)
            _lib.call("bjx_dense_matmul", stream, N, D, t.data_ptr(), U_t.data_ptr(), y.data_ptr())
        else:
            y = t
        logp_y, g_y = eval_logdensity(vg, y)
        if dense:
            U_y, U_grad_y = _rotate(y, U, U_t), _rotate(g_y, U, U_t)
        else:
            U_y, U_grad_y = y, g_y

        logp_new, acc_rate = torch.empty_like(logp_x), torch.empty_like(logp_x)
        is_acc = torch.empty(N, dtype=torch.bool, device=dev)  # one byte per flag, 0 / 1: written as uint8
        U_x_new, U_grad_x_new = torch.empty_like(x), torch.empty_like(x)
        if dense:
            x_new, g_new = torch.empty_like(x), torch.empty_like(x)
            pos = [x.data_ptr(), g_x.data_ptr(), y.data_ptr(), g_y.data_ptr(), x_new.data_ptr(), g_new.data_ptr()]
        else:
            x_new, g_new = U_x_new, U_grad_x_new
            pos = [None] * 6
        _lib.call("bjx_mgrad_finish", stream, k0, k1, off, fold, N, D, dlt, _lib.ptr(dlt_pc), gamma.data_ptr(),
                  pos[0], logp_x.data_ptr(), pos[1], U_x.data_ptr(), U_grad_x.data_ptr(), pos[2], logp_y.data_ptr(),
                  pos[3], U_y.data_ptr(), U_grad_y.data_ptr(), pos[4], logp_new.data_ptr(), pos[5],
                  U_x_new.data_ptr(), U_grad_x_new.data_ptr(), acc_rate.data_ptr(), is_acc.data_ptr())
        return (MarginalState(x_new, logp_new, g_new, U_x_new, U_grad_x_new),
                MarginalInfo(acc_rate, is_acc, MarginalState(y, logp_y, g_y, U_y, U_grad_y)))

    return kernel


def as_top_level_api(logdensity_fn: Callable, covariance=None, mean=None, cov_svd: CovarianceSVD | None = None,
                     step_size=1.0, *, chain_offset: int = 0) -> SamplingAlgorithm:
    """blackjax/mcmc/marginal_latent_gaussian.py ``as_top_level_api``: ``init(position)``, ``step(rng_key, state)``.
    ``covariance``: ``(D,)`` or ``(D, D)``, or give its factorisation ``cov_svd``; ``mean``: ``(D,)`` or a scalar."""
    if cov_svd is None:
        if covariance is None:
            raise ValueError("To initialize the MGrad kernel, either covariance or cov_svd must be passed.")
        cov = _check_covariance(covariance)
        _check_mean(mean, int(cov.shape[0]))  # shape errors come before the factorisation
        cov_svd = svd_from_covariance(cov)
    D = _check_svd(cov_svd)
    mean = _check_mean(mean, D)
    U, gamma, U_t = cov_svd
    if not bool((gamma.detach().cpu() > 0).all()):
        raise ValueError("the covariance is not positive definite: cov_svd.Gamma has a non-positive entry")
    if mean is not None:
        logdensity_fn = _MeanShifted(logdensity_fn, _shift(cov_svd, mean))
    kernel = build_kernel(cov_svd)

    def init_fn(position, rng_key=None):
        del rng_key
        if isinstance(position, torch.Tensor) and position.ndim == 2 and position.shape[1] != D:
            raise ValueError(f"the prior has {D} dims, position has {position.shape[1]}")
        return init(position, logdensity_fn, U_t)

    def step_fn(rng_key, state):
        return kernel(rng_key, state, logdensity_fn, step_size, chain_offset=chain_offset)

    return SamplingAlgorithm(init_fn, step_fn)
