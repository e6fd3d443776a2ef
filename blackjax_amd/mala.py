"""Batched Metropolis-adjusted Langevin algorithm on MI355X behind the ``blackjax.mala`` API surface.

Mirrors blackjax/mcmc/mala.py: ``MALAState``, ``MALAInfo``, ``init``, ``build_kernel`` (``transition_energy`` and
``kernel``) and ``as_top_level_api``; the proposal is one step of mcmc/diffusions.py::overdamped_langevin and the
accept is mcmc/proposal.py::compute_asymmetric_acceptance_ratio + ``static_binomial_sampling`` on
``safe_energy_diff``.  One gradient per transition, no momentum, no metric: the cheapest gradient-based sampler of
the reference and the usual inner kernel of tempered SMC.

The chain axis is native; chain ``i`` of ``step(rng_key, state)`` reproduces the reference's single-chain
``step(jax.random.split(rng_key, N)[chain_offset + i], state_i)``.  ``step_size`` may be a per-chain ``(N,)`` tensor.
Like every RNG-dependent part of the package, parity with a real JAX run is unpinned; the
arithmetic is held against a NumPy restatement of the reference (tests/mala_restatement.py).

The arithmetic runs in libbjxhip (include/bjx_hip.h, "MALA"); this module sequences
propose (one launch) -> user callable -> finish (one launch).
"""
from __future__ import annotations

from typing import Callable, NamedTuple

import torch

from . import _lib
from ._util import check_batch, eval_logdensity, step_size_args, value_and_grad
from .base import SamplingAlgorithm
from .random import key_spec

__all__ = ["MALAState", "MALAInfo", "init", "build_kernel", "as_top_level_api"]


class MALAState(NamedTuple):
    """blackjax/mcmc/mala.py ``MALAState``, batched: (N, D), (N,), (N, D)."""

    position: torch.Tensor
    logdensity: torch.Tensor
    logdensity_grad: torch.Tensor


class MALAInfo(NamedTuple):
    """blackjax/mcmc/mala.py ``MALAInfo``, batched: (N,) float32, (N,) bool."""

    acceptance_rate: torch.Tensor
    is_accepted: torch.Tensor


def init(position: torch.Tensor, logdensity_fn: Callable) -> MALAState:
    """blackjax/mcmc/mala.py ``init``: the log-density and its gradient at the initial positions."""
    position = check_batch(position, "position")
    if position.ndim != 2:
        raise ValueError(f"position must be (n_chains, dim), got {tuple(position.shape)}")
    logp, grad = eval_logdensity(value_and_grad(logdensity_fn), position)
    return MALAState(position, logp, grad)


def build_kernel():
    """blackjax/mcmc/mala.py ``build_kernel``."""

    def kernel(rng_key, state: MALAState, logdensity_fn: Callable, step_size, *, chain_offset: int = 0):
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
        off = int(chain_offset)
        q1 = torch.empty_like(q0)
        _lib.call("bjx_mala_propose", _lib.current_stream(), k0, k1, off, fold, N, D, tau, _lib.ptr(tau_pc),
                  q0.data_ptr(), g0.data_ptr(), q1.data_ptr())
        logp1, g1 = eval_logdensity(vg, q1)
        q_new, g_new, logp_new = torch.empty_like(q0), torch.empty_like(q0), torch.empty_like(logp0)
        acc_rate = torch.empty_like(logp0)
        is_acc = torch.empty(N, dtype=torch.bool, device=dev)  # one byte per flag, 0 / 1: written as uint8
        _lib.call("bjx_mala_finish", _lib.current_stream(), k0, k1, off, fold, N, D, tau, _lib.ptr(tau_pc),
                  q0.data_ptr(), logp0.data_ptr(), g0.data_ptr(), q1.data_ptr(), logp1.data_ptr(), g1.data_ptr(),
                  q_new.data_ptr(), logp_new.data_ptr(), g_new.data_ptr(), acc_rate.data_ptr(), is_acc.data_ptr())
        return MALAState(q_new, logp_new, g_new), MALAInfo(acc_rate, is_acc)

    return kernel


def as_top_level_api(logdensity_fn: Callable, step_size, *, chain_offset: int = 0) -> SamplingAlgorithm:
    """blackjax/mcmc/mala.py ``as_top_level_api``: ``init(position)``, ``step(rng_key, state)``."""
    kernel = build_kernel()

    def init_fn(position, rng_key=None):
        del rng_key
        return init(position, logdensity_fn)

    def step_fn(rng_key, state):
        return kernel(rng_key, state, logdensity_fn, step_size, chain_offset=chain_offset)

    return SamplingAlgorithm(init_fn, step_fn)
