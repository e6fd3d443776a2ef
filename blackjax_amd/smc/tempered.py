"""Tempered SMC on MI355X behind the ``blackjax.tempered_smc`` API surface.

Mirrors blackjax/smc/tempered.py: ``TemperedSMCState``, ``init``, ``build_kernel`` and ``as_top_level_api``.  One
step from temperature ``lam_old`` to ``lam_new`` (smc/base.py::step as called by smc/tempered.py::build_kernel):

1. ``updating_key, resampling_key = split(rng_key, 2)``;
2. ancestors from the INCOMING weights, rows gathered out of place;
3. ``num_mcmc_steps`` transitions of ``mcmc_step_fn`` on ``logprior + lam_old * loglikelihood`` (the OLD temperature),
   particle ``i`` keyed ``split(split(updating_key, N)[i], num_mcmc_steps)[t]``;
4. weights ``exp(lw - logsumexp(lw))`` with ``lw = (lam_new - lam_old) * loglikelihood`` at the moved particles,
   ``log_likelihood_increment = logsumexp(lw) - log N``.

The tempered log-density is ONE object per algorithm: ``value_and_grad`` of the prior and of the likelihood are taken
once, and a small kernel (``bjx_smc_temper``) combines their outputs with the temperature read from device memory.
No temperature is baked into a traced or recorded function and no new closure reaches ``value_and_grad`` per step.
The temperature, the increment and the weights stay on the device: the only host reads are the caller's own
(``while state.lmbda < 1`` reads 4 bytes).

A particle whose log-likelihood is ``-inf`` or NaN gets weight 0 (the weighting rule of
``csrc/bjx_smc_dev.h``).  If EVERY particle is like that (and the temperature moved) the weights are NaN and the
increment is ``-inf``; no host check is made for it.  With ``lam_new == lam_old`` the weights are uniform whatever the
log-likelihoods are.

``update_strategy`` decides how the resampled particles are moved and how many are resampled: ``update_and_take_last``
(all ``N``, the last of ``num_mcmc_steps`` states kept) or ``blackjax_amd.smc.waste_free.waste_free_smc(N, p)``
(``N / p`` ancestors, every state kept; ``SMCInfo.ancestors`` is then ``(N / p,)``).  The parameters of the move can
be re-estimated between temperatures with ``blackjax_amd.smc.inner_kernel_tuning``, or carried as one value per
particle and adapted before every step with ``blackjax_amd.smc.pretuning``.

Out of scope: partial-posteriors (persistent sampling is ``blackjax_amd.smc.persistent_sampling``), pytrees of
particles, and sharding the particles across GPUs (resampling is global: there is no ``chain_offset`` here).
"""
from __future__ import annotations

from typing import Callable, NamedTuple

import torch

from .. import _lib
from .._util import eval_logdensity, eval_value, is_capturable, value_and_grad
from ..base import SamplingAlgorithm
from ..random import split
from . import base

__all__ = ["TemperedSMCState", "TemperedLogDensity", "init", "build_kernel", "as_top_level_api"]


class TemperedSMCState(NamedTuple):
    """blackjax/smc/tempered.py ``TemperedSMCState``: (N, D) particles, (N,) weights, 0-d device temperature."""

    particles: torch.Tensor
    weights: torch.Tensor
    lmbda: torch.Tensor


def init(particles) -> TemperedSMCState:
    """blackjax/smc/tempered.py ``init``: uniform weights at temperature 0."""
    x = base.check_particles(particles)
    n = x.shape[0]
    return TemperedSMCState(x, torch.full((n,), 1.0 / n, dtype=torch.float32, device=x.device),
                            torch.zeros((), dtype=torch.float32, device=x.device))


class TemperedLogDensity:
    """``q -> (logprior(q) + lam * loglikelihood(q), its gradient)`` with ``lam`` held in device memory
    (smc/tempered.py::build_kernel, tempered_logposterior_fn).  Built once per algorithm; ``set_temperature`` copies a
    device scalar into the buffer the combine kernel reads, so a recorded or traced evaluation stays valid at every
    temperature.  Recordable exactly when both user callables are."""

    _bjx_returns_pair = True
    _bjx_value_and_grad = True

    def __init__(self, logprior_fn: Callable, loglikelihood_fn: Callable):
        self.logprior_fn, self.loglikelihood_fn = logprior_fn, loglikelihood_fn
        self.logprior_vg = value_and_grad(logprior_fn)
        self.loglikelihood_vg = value_and_grad(loglikelihood_fn)
        self._bjx_capturable = is_capturable(logprior_fn) and is_capturable(loglikelihood_fn)
        self._lam: dict = {}  # device -> the 0-d buffer every evaluation on that device reads

    def temperature(self, device) -> torch.Tensor:
        buf = self._lam.get(device)
        if buf is None:
            buf = self._lam[device] = torch.zeros((), dtype=torch.float32, device=device)
        return buf

    def set_temperature(self, lmbda: torch.Tensor) -> None:
        self.temperature(lmbda.device).copy_(lmbda)

    def loglikelihood(self, q: torch.Tensor) -> torch.Tensor:
        return eval_logdensity(self.loglikelihood_vg, q)[0]

    def __call__(self, q: torch.Tensor):
        lp, gp = eval_logdensity(self.logprior_vg, q)
        ll, gl = eval_logdensity(self.loglikelihood_vg, q)
        n, d = q.shape
        logp, grad = torch.empty_like(lp), torch.empty_like(gp)
        _lib.call("bjx_smc_temper", _lib.current_stream(), n, d, self.temperature(q.device).data_ptr(), lp.data_ptr(),
                  gp.data_ptr(), ll.data_ptr(), gl.data_ptr(), logp.data_ptr(), grad.data_ptr())
        return logp, grad

    def _bjx_value(self, q: torch.Tensor) -> torch.Tensor:
        """The value alone (``_util.eval_value``): both callables evaluated value-only, combined by
        ``bjx_smc_temper_value`` with the arithmetic ``bjx_smc_temper`` uses for ``logp`` -- bit-equal to
        ``self(q)[0]`` whenever the callables' values are.  What a gradient-free inner kernel pays per move."""
        lp = eval_value(self.logprior_fn, q)
        ll = eval_value(self.loglikelihood_fn, q)
        logp = torch.empty_like(lp)
        _lib.call("bjx_smc_temper_value", _lib.current_stream(), q.shape[0], self.temperature(q.device).data_ptr(),
                  lp.data_ptr(), ll.data_ptr(), logp.data_ptr())
        return logp


def build_kernel(logprior_fn: Callable, loglikelihood_fn: Callable, mcmc_step_fn: Callable, mcmc_init_fn: Callable,
                 resampling_fn: Callable, update_strategy: Callable = base.update_and_take_last):
    """blackjax/smc/tempered.py ``build_kernel``: ``kernel(rng_key, state, num_mcmc_steps, lmbda, mcmc_parameters)``.
    ``mcmc_step_fn`` is a kernel of this package (``blackjax_amd.mala.build_kernel()`` ...), ``mcmc_init_fn`` its
    ``init``; ``mcmc_parameters`` is a dict of keyword arguments (scalars shared, ``(N,)`` tensors per particle)."""
    tempered = TemperedLogDensity(logprior_fn, loglikelihood_fn)
    resample = getattr(resampling_fn, "_bjx_trusted", resampling_fn)

    def kernel(rng_key, state: TemperedSMCState, num_mcmc_steps: int, lmbda, mcmc_parameters: dict):
        x = base.check_particles(state.particles, "state.particles")
        n = x.shape[0]
        w = base.check_weights(state.weights, n, "state.weights")
        lam_old = base.device_scalar(state.lmbda, x.device)
        lam_new = base.device_scalar(lmbda, x.device)
        keys = split(rng_key, 2)
        updating_key, resampling_key = keys[0], keys[1]
        update, num_resampled = update_strategy(mcmc_init_fn, tempered, mcmc_step_fn, num_mcmc_steps, n)
        ancestors = resample(resampling_key, w, num_resampled)
        x = base.gather(x, ancestors)
        tempered.set_temperature(lam_old)
        x, update_info = update(updating_key, x, mcmc_parameters)
        weights, increment, lam = base.reweight(tempered.loglikelihood(x), lam_old, lam_new)
        return TemperedSMCState(x, weights, lam), base.SMCInfo(ancestors, increment, update_info)

    kernel.tempered_logdensity = tempered
    return kernel


def as_top_level_api(logprior_fn: Callable, loglikelihood_fn: Callable, mcmc_step_fn: Callable,
                     mcmc_init_fn: Callable, mcmc_parameters: dict, resampling_fn: Callable,
                     num_mcmc_steps: int = 10,
                     update_strategy: Callable = base.update_and_take_last) -> SamplingAlgorithm:
    """blackjax/smc/tempered.py ``as_top_level_api``: ``init(particles)``, ``step(rng_key, state, lmbda)``.
    ``update_strategy=waste_free_smc(N, p)`` goes with ``num_mcmc_steps=None``."""
    kernel = build_kernel(logprior_fn, loglikelihood_fn, mcmc_step_fn, mcmc_init_fn, resampling_fn, update_strategy)

    def init_fn(particles, rng_key=None):
        del rng_key
        return init(particles)

    def step_fn(rng_key, state, lmbda):
        return kernel(rng_key, state, num_mcmc_steps, lmbda, mcmc_parameters)

    return SamplingAlgorithm(init_fn, step_fn)
