"""Waste-free SMC (Dau & Chopin 2022) behind ``blackjax.smc.waste_free``: every intermediate state of the move is a
particle of the next generation.

Mirrors blackjax/smc/waste_free.py ``waste_free_smc(n_particles, p)`` and ``update_waste_free``.  Only
``M = n_particles // p`` ancestors are resampled; each of the ``M`` chains makes ``p - 1`` transitions and all
``M + M (p - 1) = N`` states are kept, in the reference's layout: rows ``[0, M)`` are the resampled particles, row
``M + i (p - 1) + t`` is chain ``i`` after transition ``t + 1`` (its reshape of the scanned ``(M, p - 1, D)`` states
followed by its concatenation).  Chain ``i`` at transition ``t`` is keyed ``split(split(rng_key, M)[i], p - 1)[t]``
(``ChainMajorKey``).

Each transition's positions are stored straight into their rows of the preallocated ``(N, D)`` output by a strided
row store (``bjx_smc_scatter_rows``): there is no ``(M, p - 1, D)`` temporary, no concatenation and no host read.
``p = 1`` (no transition at all) is not carried: ``p >= 2``.
"""
from __future__ import annotations

from typing import Callable

import torch

from .. import _lib
from ..random import ChainMajorKey
from . import base

__all__ = ["waste_free_smc", "update_waste_free", "scatter_rows"]


def scatter_rows(x: torch.Tensor, row0: int, row_stride: int, out: torch.Tensor) -> torch.Tensor:
    """``out[row0 + i * row_stride] = x[i]`` for every row of ``x`` (``bjx_smc_scatter_rows``); the other rows of
    ``out`` keep their bytes.  ``x`` (M, D) and ``out`` (R, D) are contiguous float32 tensors on one device."""
    x = base.check_particles(x, "x")
    dst = base.check_particles(out, "out")
    if dst.data_ptr() != out.data_ptr():
        raise ValueError("out must be a contiguous float32 tensor: the rows are stored in place")
    m, d = x.shape
    row0, row_stride = int(row0), int(row_stride)
    if out.shape[1] != d or out.device != x.device:
        raise ValueError(f"out must be (rows, {d}) on {x.device}, got {tuple(out.shape)} on {out.device}")
    if row0 < 0 or row_stride < 1 or row0 + (m - 1) * row_stride >= out.shape[0]:
        raise ValueError(f"rows {row0} + i * {row_stride}, i < {m}, do not fit the {out.shape[0]} rows of out")
    _lib.call("bjx_smc_scatter_rows", _lib.current_stream(), m, d, x.data_ptr(), row0, row_stride, out.data_ptr())
    return out


def update_waste_free(mcmc_init_fn: Callable, logposterior_fn: Callable, mcmc_step_fn: Callable, n_particles: int,
                      p: int, num_resampled: int, num_mcmc_steps=None):
    """blackjax/smc/waste_free.py ``update_waste_free`` -> ``(update, num_resampled)``.  ``update(rng_key, position
    (M, D), mcmc_parameters) -> ((N, D) particles, infos)``; ``infos`` is the tuple of the ``p - 1`` transitions'
    infos in step order, each with ``(M,)`` fields.  Per-particle ``mcmc_parameters`` are ``(M,)`` tensors."""
    if num_mcmc_steps is not None:
        raise ValueError("Can't use waste free SMC with a num_mcmc_steps parameter, set num_mcmc_steps = None")
    n_particles, p, num_resampled = int(n_particles), int(p), int(num_resampled)

    def update(rng_key, position, mcmc_parameters):
        x = base.check_particles(position, "position")
        if x.shape[0] != num_resampled:
            raise ValueError(f"waste-free SMC moves {num_resampled} resampled particles, got {x.shape[0]}")
        out = torch.empty((n_particles, x.shape[1]), dtype=torch.float32, device=x.device)
        scatter_rows(x, 0, 1, out)
        state = mcmc_init_fn(x, logposterior_fn)
        infos = []
        for t in range(p - 1):
            state, info = mcmc_step_fn(ChainMajorKey(rng_key, t), state, logposterior_fn, **mcmc_parameters)
            scatter_rows(state.position, num_resampled + t, p - 1, out)
            infos.append(info)
        return out, tuple(infos)

    return update, num_resampled


def waste_free_smc(n_particles: int, p: int) -> Callable:
    """blackjax/smc/waste_free.py ``waste_free_smc``: an ``update_strategy`` for ``tempered_smc`` /
    ``adaptive_tempered_smc`` (and ``inner_kernel_tuning`` around them), to be used with ``num_mcmc_steps=None``.
    ``n_particles`` must be a multiple of ``p >= 2``."""
    n_particles, p = int(n_particles), int(p)
    if p < 2:
        raise ValueError(f"waste-free SMC needs p >= 2 (p - 1 transitions per resampled particle), got p = {p}")
    if n_particles < 1 or n_particles % p != 0:
        raise ValueError(f"p must be a divider of n_particles, got n_particles = {n_particles} and p = {p}")
    num_resampled = n_particles // p

    def strategy(mcmc_init_fn, logposterior_fn, mcmc_step_fn, num_mcmc_steps, n_particles_of_state):
        if int(n_particles_of_state) != n_particles:
            raise ValueError(f"waste_free_smc was built for {n_particles} particles, the state holds "
                             f"{n_particles_of_state}")
        return update_waste_free(mcmc_init_fn, logposterior_fn, mcmc_step_fn, n_particles, p, num_resampled,
                                 num_mcmc_steps)

    strategy.n_particles, strategy.p, strategy.num_resampled = n_particles, p, num_resampled
    return strategy
