"""Adaptive tempered SMC on MI355X behind the ``blackjax.adaptive_tempered_smc`` API surface.

Mirrors blackjax/smc/adaptive_tempered.py ``build_kernel`` (``compute_delta``) and ``as_top_level_api``; the state
and ``init`` are those of smc/tempered.py.  Before the tempered step the next temperature is solved for on the
incoming particles: the largest increment ``delta <= 1 - lmbda`` whose effective sample size is at least
``target_ess * N`` (smc/ess.py::ess_solver with smc/solver.py::dichotomy).  The bisection is one device launch
(``bjx_smc_ess_solve``); when the whole remaining interval is taken the new temperature is exactly 1.0, so
``while state.lmbda < 1`` terminates.  If no increment reaches the target -- every particle of weight 0, say --
``delta`` is 0 and the temperature does not move; no host check is made for it.

Out of scope: as for ``blackjax_amd.smc.tempered``.
"""
from __future__ import annotations

from typing import Callable

import torch

from ..base import SamplingAlgorithm
from . import base, solver, tempered

__all__ = ["init", "build_kernel", "as_top_level_api"]

init = tempered.init


def build_kernel(logprior_fn: Callable, loglikelihood_fn: Callable, mcmc_step_fn: Callable, mcmc_init_fn: Callable,
                 resampling_fn: Callable, target_ess: float, root_solver: Callable = solver.dichotomy,
                 update_strategy: Callable = base.update_and_take_last):
    """blackjax/smc/adaptive_tempered.py ``build_kernel``: ``kernel(rng_key, state, num_mcmc_steps,
    mcmc_parameters)``.  ``root_solver(loglikelihood, target_ess, max_delta) -> delta`` works on device tensors.
    The solve sees the log-likelihood of all ``N`` incoming particles whatever ``update_strategy`` resamples."""
    tempered_kernel = tempered.build_kernel(logprior_fn, loglikelihood_fn, mcmc_step_fn, mcmc_init_fn, resampling_fn,
                                            update_strategy)
    logdensity = tempered_kernel.tempered_logdensity

    def kernel(rng_key, state: tempered.TemperedSMCState, num_mcmc_steps: int, mcmc_parameters: dict):
        x = base.check_particles(state.particles, "state.particles")
        lam_old = base.device_scalar(state.lmbda, x.device)
        ll = logdensity.loglikelihood(x)
        if root_solver is solver.dichotomy:
            _, lam_new = solver.next_temperature(ll, target_ess, lam_old)
        else:
            max_delta = 1.0 - lam_old
            delta = root_solver(ll, target_ess, max_delta)
            lam_new = torch.where(delta >= max_delta, torch.ones_like(lam_old), lam_old + delta)
        return tempered_kernel(rng_key, state, num_mcmc_steps, lam_new, mcmc_parameters)

    kernel.tempered_logdensity = logdensity
    return kernel


def as_top_level_api(logprior_fn: Callable, loglikelihood_fn: Callable, mcmc_step_fn: Callable,
                     mcmc_init_fn: Callable, mcmc_parameters: dict, resampling_fn: Callable, target_ess: float,
                     root_solver: Callable = solver.dichotomy, num_mcmc_steps: int = 10,
                     update_strategy: Callable = base.update_and_take_last) -> SamplingAlgorithm:
    """blackjax/smc/adaptive_tempered.py ``as_top_level_api``: ``init(particles)``, ``step(rng_key, state)``.
    ``update_strategy=waste_free_smc(N, p)`` goes with ``num_mcmc_steps=None``."""
    kernel = build_kernel(logprior_fn, loglikelihood_fn, mcmc_step_fn, mcmc_init_fn, resampling_fn, target_ess,
                          root_solver, update_strategy)

    def init_fn(particles, rng_key=None):
        del rng_key
        return init(particles)

    def step_fn(rng_key, state):
        return kernel(rng_key, state, num_mcmc_steps, mcmc_parameters)

    return SamplingAlgorithm(init_fn, step_fn)
