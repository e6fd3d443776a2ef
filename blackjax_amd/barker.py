"""Batched Barker-proposal sampler on MI355X behind the ``blackjax.barker_proposal`` API surface.

Mirrors blackjax/mcmc/barker.py: ``BarkerState``, ``BarkerInfo``, ``init``, ``build_kernel`` (``_barker_sample_nd``,
``_barker_logpdf`` and ``kernel``) and ``as_top_level_api``; the accept is
mcmc/proposal.py::compute_asymmetric_acceptance_ratio + ``static_binomial_sampling`` on ``safe_energy_diff``
(Livingstone & Zanella 2022).  One gradient per transition like ``mala``, but every coordinate moves by ``+z`` or
``-z`` with the probability ``expit(z g)`` its gradient gives, which keeps the sampler usable at a step size that is
far off -- the property a warm-up needs.  The kernel takes ``(rng_key, state, logdensity_fn, step_size,
inverse_mass_matrix)``, so ``window_adaptation(blackjax_amd.barker, ...)`` tunes a per-chain step size and a per-chain
diagonal metric for it (a target acceptance rate of about 0.4 is the usual choice).

The chain axis is native; chain ``i`` of ``step(rng_key, state)`` follows the reference's single-chain
``step(jax.random.split(rng_key, N)[chain_offset + i], state_i)``.  ``step_size`` may be a per-chain ``(N,)`` tensor;
``inverse_mass_matrix`` is ``None`` (ones), a shared ``(D,)`` diagonal or per-chain ``(N, D)`` diagonals
(``metrics.PerChainDiag`` / ``PerChainDiagTensor``).  Dense preconditioning is not implemented.  Like every
RNG-dependent part of the package, parity with a real JAX run is unpinned; the arithmetic is held
against a NumPy restatement (tests/barker_restatement.py).

The arithmetic runs in libbjxhip (include/bjx_hip.h, "Barker"); this module sequences
propose (one launch) -> user callable -> finish (one launch).
"""
from __future__ import annotations

from typing import Callable, NamedTuple

import torch

from . import _lib, metrics
from ._util import check_batch, eval_logdensity, step_size_args, value_and_grad
from .base import SamplingAlgorithm
from .random import key_spec

__all__ = ["BarkerState", "BarkerInfo", "init", "build_kernel", "as_top_level_api"]


class BarkerState(NamedTuple):
    """blackjax/mcmc/barker.py ``BarkerState``, batched: (N, D), (N,), (N, D)."""

    position: torch.Tensor
    logdensity: torch.Tensor
    logdensity_grad: torch.Tensor


class BarkerInfo(NamedTuple):
    """blackjax/mcmc/barker.py ``BarkerInfo``, batched: (N,) float32, (N,) bool, the proposed ``BarkerState``."""

    acceptance_rate: torch.Tensor
    is_accepted: torch.Tensor
    proposal: BarkerState


def init(position: torch.Tensor, logdensity_fn: Callable) -> BarkerState:
    """blackjax/mcmc/barker.py ``init``: the log-density and its gradient at the initial positions."""
    position = check_batch(position, "position")
    if position.ndim != 2:
        raise ValueError(f"position must be (n_chains, dim), got {tuple(position.shape)}")
    logp, grad = eval_logdensity(value_and_grad(logdensity_fn), position)
    return BarkerState(position, logp, grad)


_DENSE = ("barker: a dense inverse_mass_matrix is not implemented; pass None, a shared (D,) diagonal or per-chain "
          "(N, D) diagonals (metrics.PerChainDiag / PerChainDiagTensor)")


def _diag_imm(inverse_mass_matrix, n_chains: int, dim: int, device):
    """-> (contiguous fp32 device tensor or None, row stride): the diagonal forms of ``metrics.default_metric``."""
    imm = inverse_mass_matrix
    if imm is None:
        return None, 0
    if isinstance(imm, metrics.Metric):
        if imm.kind != "diag":
            raise NotImplementedError(_DENSE)
        per_chain, imm = imm.imm_stride != 0, imm.imm
    else:
        per_chain = False
        if isinstance(imm, metrics.PerChainDiag):
            per_chain, imm = True, imm.imm
        if isinstance(imm, metrics.PerChainDiagTensor):
            per_chain, imm = True, imm.as_subclass(torch.Tensor)
    imm = torch.as_tensor(imm, dtype=torch.float32, device=device)
    if imm.ndim == 1:
        if imm.shape[0] != dim:
            raise ValueError(f"inverse_mass_matrix has {imm.shape[0]} entries, position has {dim}")
        return imm.contiguous(), 0
    if imm.ndim == 2 and (per_chain or (imm.shape[0] == n_chains and imm.shape[0] != imm.shape[1])):
        if imm.shape != (n_chains, dim):
            raise ValueError(f"per-chain inverse_mass_matrix must be ({n_chains}, {dim}), got {tuple(imm.shape)}")
        return imm.contiguous(), dim
    if (imm.ndim == 2 and imm.shape[0] == imm.shape[1]) or (imm.ndim == 3 and imm.shape[1] == imm.shape[2]):
        raise NotImplementedError(_DENSE)
    raise ValueError(f"inverse_mass_matrix must be (D,) or (N, D), got {tuple(imm.shape)}")


def build_kernel():
    """blackjax/mcmc/barker.py ``build_kernel``."""

    def kernel(rng_key, state: BarkerState, logdensity_fn: Callable, step_size, inverse_mass_matrix=None, *,
               chain_offset: int = 0):
        q0 = check_batch(state.position, "state.position")
        logp0 = check_batch(state.logdensity, "state.logdensity")
        g0 = check_batch(state.logdensity_grad, "state.logdensity_grad")
        if q0.ndim != 2:
            raise ValueError(f"state.position must be (n_chains, dim), got {tuple(q0.shape)}")
        N, D = q0.shape
        dev = q0.device
        k0, k1, fold = key_spec(rng_key)
        vg = value_and_grad(logdensity_fn)
        tau, tau_pc = step_size_args(step_size, N, dev)
        imm, imm_stride = _diag_imm(inverse_mass_matrix, N, D, dev)
        off = int(chain_offset)
        q1 = torch.empty_like(q0)
        _lib.call("bjx_barker_propose", _lib.current_stream(), k0, k1, off, fold, N, D, tau, _lib.ptr(tau_pc),
                  _lib.ptr(imm), imm_stride, q0.data_ptr(), g0.data_ptr(), q1.data_ptr())
        logp1, g1 = eval_logdensity(vg, q1)
        q_new, g_new, logp_new = torch.empty_like(q0), torch.empty_like(q0), torch.empty_like(logp0)
        acc_rate = torch.empty_like(logp0)
        is_acc = torch.empty(N, dtype=torch.bool, device=dev)  # one byte per flag, 0 / 1: written as uint8
        _lib.call("bjx_barker_finish", _lib.current_stream(), k0, k1, off, fold, N, D, q0.data_ptr(),
                  logp0.data_ptr(), g0.data_ptr(), q1.data_ptr(), logp1.data_ptr(), g1.data_ptr(), q_new.data_ptr(),
                  logp_new.data_ptr(), g_new.data_ptr(), acc_rate.data_ptr(), is_acc.data_ptr())
        return BarkerState(q_new, logp_new, g_new), BarkerInfo(acc_rate, is_acc, BarkerState(q1, logp1, g1))

    return kernel


def as_top_level_api(logdensity_fn: Callable, step_size, inverse_mass_matrix=None, *,
                     chain_offset: int = 0) -> SamplingAlgorithm:
    """blackjax/mcmc/barker.py ``as_top_level_api``: ``init(position)``, ``step(rng_key, state)``."""
    kernel = build_kernel()

    def init_fn(position, rng_key=None):
        del rng_key
        return init(position, logdensity_fn)

    def step_fn(rng_key, state):
        return kernel(rng_key, state, logdensity_fn, step_size, inverse_mass_matrix, chain_offset=chain_offset)

    return SamplingAlgorithm(init_fn, step_fn)
