"""The generic SMC step behind ``blackjax.smc.base``: resample, gather, update, reweight.

Mirrors blackjax/smc/base.py: ``SMCState``, ``SMCInfo``, ``init``, ``step``, ``extend_params`` and
``update_and_take_last``.  Particles are one ``(N, D)`` float32 device tensor (the chain axis of every other sampler
of this package); pytrees of particles are out of scope.  The row gather, the log-sum-exp normalisation and the
likelihood increment run in libbjxhip (include/bjx_hip.h, "SMC"); nothing here reads a value back to the host.
"""
from __future__ import annotations

from typing import Callable, NamedTuple

import torch

from .. import _lib
from .._util import check_batch
from ..random import ChainMajorKey, split

__all__ = ["SMCState", "SMCInfo", "init", "step", "gather", "reweight", "normalize", "extend_params",
           "update_and_take_last"]


class SMCState(NamedTuple):
    """blackjax/smc/base.py ``SMCState``: (N, D) particles, (N,) normalised weights, the update's parameters."""

    particles: torch.Tensor
    weights: torch.Tensor
    update_parameters: object


class SMCInfo(NamedTuple):
    """blackjax/smc/base.py ``SMCInfo``: (N,) int32 ancestors, 0-d log-likelihood increment, the update's info."""

    ancestors: torch.Tensor
    log_likelihood_increment: torch.Tensor
    update_info: object


def check_particles(particles, name: str = "particles") -> torch.Tensor:
    x = check_batch(particles, name)
    if x.ndim != 2:
        raise ValueError(f"{name} must be (n_particles, dim), got {tuple(x.shape)}")
    if x.shape[0] < 1:
        raise ValueError(f"{name} must hold at least one particle")
    return x


def check_weights(weights, n: int, name: str = "weights") -> torch.Tensor:
    w = check_batch(weights, name)
    if w.shape != (n,):
        raise ValueError(f"{name} must have shape ({n},), got {tuple(w.shape)}")
    return w


def device_scalar(value, device) -> torch.Tensor:
    """A 0-d float32 tensor on ``device`` (a Python number is written with one fill launch; nothing is read)."""
    if isinstance(value, torch.Tensor):
        if value.numel() != 1:
            raise ValueError(f"expected a scalar, got shape {tuple(value.shape)}")
        return value.detach().to(device=device, dtype=torch.float32).reshape(())
    return torch.full((), float(value), dtype=torch.float32, device=device)


def init(particles, init_update_params=None) -> SMCState:
    """blackjax/smc/base.py ``init``: uniform weights."""
    x = check_particles(particles)
    n = x.shape[0]
    return SMCState(x, torch.full((n,), 1.0 / n, dtype=torch.float32, device=x.device), init_update_params)


def gather(particles, ancestors) -> torch.Tensor:
    """``particles[ancestors]`` out of place (``bjx_smc_gather``): (N, D), (M,) int32 -> (M, D)."""
    x = check_particles(particles)
    if not isinstance(ancestors, torch.Tensor):
        raise TypeError(f"ancestors must be a torch.Tensor, got {type(ancestors)}")
    if not ancestors.is_cuda:
        raise RuntimeError(f"ancestors lives on {ancestors.device}: blackjax_amd runs on ROCm device tensors only")
    if ancestors.dtype != torch.int32 or ancestors.ndim != 1:
        raise ValueError(f"ancestors must be a 1-d int32 tensor, got {ancestors.dtype} {tuple(ancestors.shape)}")
    a = ancestors.contiguous()
    n, d = x.shape
    out = torch.empty((a.shape[0], d), dtype=torch.float32, device=x.device)
    _lib.call("bjx_smc_gather", _lib.current_stream(), n, a.shape[0], d, x.data_ptr(), a.data_ptr(), out.data_ptr())
    return out


def reweight(loglikelihood, lam_old, lam_new):
    """``bjx_smc_reweight``: log-weights ``(lam_new - lam_old) * loglikelihood`` -> (normalised weights (N,),
    log-likelihood increment 0-d, the new temperature 0-d).  ``lam_old`` / ``lam_new`` are 0-d device tensors."""
    ll = check_batch(loglikelihood, "loglikelihood")
    if ll.ndim != 1 or ll.shape[0] < 1:
        raise ValueError(f"loglikelihood must be (n_particles,), got {tuple(ll.shape)}")
    dev = ll.device
    lam_old, lam_new = device_scalar(lam_old, dev), device_scalar(lam_new, dev)
    w = torch.empty_like(ll)
    inc = torch.empty((), dtype=torch.float32, device=dev)
    lam = torch.empty((), dtype=torch.float32, device=dev)
    _lib.call("bjx_smc_reweight", _lib.current_stream(), ll.shape[0], ll.data_ptr(), lam_old.data_ptr(),
              lam_new.data_ptr(), w.data_ptr(), inc.data_ptr(), lam.data_ptr())
    return w, inc, lam


def normalize(log_weights):
    """blackjax/smc/base.py ``step``, the weighting: ``(exp(lw - logsumexp(lw)), logsumexp(lw) - log N)``."""
    w, inc, _ = reweight(log_weights, 0.0, 1.0)  # (1 - 0) * lw is lw exactly
    return w, inc


def step(rng_key, state: SMCState, update_fn: Callable, weight_fn: Callable, resample_fn: Callable,
         num_resampled=None):
    """blackjax/smc/base.py ``step``: ancestors from the incoming weights, gather, ``update_fn(key, particles,
    update_parameters) -> (particles, info)``, then ``weight_fn(particles) -> (N,) log-weights``, normalised."""
    x = check_particles(state.particles, "state.particles")
    w = check_weights(state.weights, x.shape[0], "state.weights")
    keys = split(rng_key, 2)
    updating_key, resampling_key = keys[0], keys[1]
    m = x.shape[0] if num_resampled is None else int(num_resampled)
    ancestors = getattr(resample_fn, "_bjx_trusted", resample_fn)(resampling_key, w, m)
    particles, update_info = update_fn(updating_key, gather(x, ancestors), state.update_parameters)
    weights, increment = normalize(weight_fn(particles))
    return SMCState(particles, weights, state.update_parameters), SMCInfo(ancestors, increment, update_info)


def extend_params(params):
    """blackjax/smc/base.py ``extend_params``.  The reference adds a leading axis of 1 to parameters shared by all
    particles so that they broadcast under its vmap; here a scalar entry IS shared and an ``(N,)`` tensor is per
    particle, so the helper the reference idiom calls returns the parameters unchanged (as a new dict)."""
    return dict(params)


def update_and_take_last(mcmc_init_fn: Callable, tempered_logposterior_fn: Callable, mcmc_step_fn: Callable,
                         num_mcmc_steps: int, n_particles: int):
    """blackjax/smc/base.py ``update_and_take_last``: ``num_mcmc_steps`` transitions of every particle, keeping the
    last state and info.  Particle ``i`` uses ``split(split(rng_key, N)[i], num_mcmc_steps)[t]`` at transition ``t``
    (``ChainMajorKey``): the key layout of the reference's vmapped per-particle scan.  Per-particle parameters are
    not resampled, as in the reference."""
    num_mcmc_steps = int(num_mcmc_steps)

    def mcmc_kernel(rng_key, position, mcmc_parameters):
        state = mcmc_init_fn(position, tempered_logposterior_fn)
        info = None
        for t in range(num_mcmc_steps):
            state, info = mcmc_step_fn(ChainMajorKey(rng_key, t), state, tempered_logposterior_fn, **mcmc_parameters)
        return state.position, info

    return mcmc_kernel, n_particles
