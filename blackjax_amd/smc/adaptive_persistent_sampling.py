"""Adaptive persistent-sampling SMC on MI355X behind the ``blackjax.adaptive_persistent_sampling_smc`` API surface.

Mirrors blackjax/smc/adaptive_persistent_sampling.py ``calculate_lambda``, ``build_kernel`` and ``as_top_level_api``;
the state and ``init`` are those of smc/persistent_sampling.py.  Before the step the next temperature is solved for on
the ``P = (iteration + 1) * N`` particles the step will weigh: the largest ``delta <= 1 - lambda_t`` whose effective
sample size ``exp(log_ess(lw(lambda_t + delta)))`` is at least ``target_ess * N``, by the house bisection of
``blackjax_amd.smc.solver.dichotomy`` (``bjx_smc_persistent_ess_solve``: 31 evaluations, each a grid-wide reduction,
the bracket kept on the device).  When the whole remaining interval is taken the new temperature is exactly 1.0, so
``while state.tempering_param < 1`` terminates.

``target_ess`` is a multiple of ``N`` and may exceed 1: the persistent set can hold more than ``N`` effective
particles.  If the target cannot be reached even at ``delta = 0`` the result is ``delta = 0`` exactly and the step adds
a slot at the SAME temperature; that raises the reachable ESS, so a later step moves.  (With ``target_ess = 2`` the
first two steps of a run do not move.)  No host check is made for it: ``max_iterations`` bounds the run.

Out of scope: as for ``blackjax_amd.smc.persistent_sampling``.
"""
from __future__ import annotations

from typing import Callable

import torch

from .. import _lib
from ..base import SamplingAlgorithm
from . import persistent_sampling, solver
from .persistent_sampling import PersistentSMCState

__all__ = ["init", "calculate_lambda", "build_kernel", "as_top_level_api"]

init = persistent_sampling.init


def _check_target(target_ess) -> float:
    target_ess = float(target_ess)
    if not target_ess > 0.0:
        raise ValueError(f"target_ess is a positive multiple of the particles per iteration, got {target_ess}")
    return target_ess


def calculate_lambda(state: PersistentSMCState, target_ess: float) -> torch.Tensor:
    """blackjax/smc/adaptive_persistent_sampling.py ``calculate_lambda``: the next temperature as a 0-d device tensor,
    exactly 1.0 when the whole of ``1 - state.tempering_param`` keeps the ESS at or above ``target_ess * N``."""
    target_ess = _check_target(target_ess)
    pll, plz, sched, t, n_terms = persistent_sampling._check_persistent(
        state.persistent_log_likelihoods, state.persistent_log_Z, state.tempering_schedule, state.iteration, True)
    n = pll.shape[1]
    P = n_terms * n
    den = persistent_sampling._denominator(pll, plz, sched, n_terms)
    delta = torch.empty((), dtype=torch.float32, device=pll.device)
    lam_new = torch.empty((), dtype=torch.float32, device=pll.device)
    _lib.call("bjx_smc_persistent_ess_solve", _lib.current_stream(), P, pll.data_ptr(), den.data_ptr(),
              n * target_ess, sched.data_ptr() + 4 * t, persistent_sampling._workspace(P, pll.device).data_ptr(),
              delta.data_ptr(), lam_new.data_ptr())
    return lam_new


def build_kernel(logprior_fn: Callable, loglikelihood_fn: Callable, mcmc_step_fn: Callable, mcmc_init_fn: Callable,
                 resampling_fn: Callable, target_ess: float, root_solver: Callable = solver.dichotomy):
    """blackjax/smc/adaptive_persistent_sampling.py ``build_kernel``: ``kernel(rng_key, state, num_mcmc_steps,
    mcmc_parameters)``.  A ``root_solver`` other than ``solver.dichotomy`` is called as ``root_solver(fun,
    target_ess, max_delta) -> delta`` with ``fun(delta) -> (P,)`` the log-weights at ``lambda_t + delta`` on the
    device, in the manner of ``blackjax_amd.smc.adaptive_tempered``."""
    target_ess = _check_target(target_ess)
    kernel_ps = persistent_sampling.build_kernel(logprior_fn, loglikelihood_fn, mcmc_step_fn, mcmc_init_fn,
                                                 resampling_fn)

    def kernel(rng_key, state: PersistentSMCState, num_mcmc_steps: int, mcmc_parameters: dict):
        if root_solver is solver.dichotomy:
            lam_new = calculate_lambda(state, target_ess)
        else:
            pll, plz, sched, t, n_terms = persistent_sampling._check_persistent(
                state.persistent_log_likelihoods, state.persistent_log_Z, state.tempering_schedule, state.iteration,
                True)
            P = n_terms * pll.shape[1]
            ll = pll.view(-1)[:P]
            den = persistent_sampling._denominator(pll, plz, sched, n_terms)
            lam_old = sched[t]
            max_delta = 1.0 - lam_old
            delta = root_solver(lambda d: (lam_old + d) * ll - den, target_ess, max_delta)
            lam_new = torch.where(delta >= max_delta, torch.ones_like(lam_old), lam_old + delta)
        return kernel_ps(rng_key, state, num_mcmc_steps, lam_new, mcmc_parameters)

    kernel.tempered_logdensity = kernel_ps.tempered_logdensity
    return kernel


def as_top_level_api(logprior_fn: Callable, loglikelihood_fn: Callable, max_iterations: int, mcmc_step_fn: Callable,
                     mcmc_init_fn: Callable, mcmc_parameters: dict, resampling_fn: Callable, target_ess: float,
                     root_solver: Callable = solver.dichotomy, num_mcmc_steps: int = 10) -> SamplingAlgorithm:
    """blackjax/smc/adaptive_persistent_sampling.py ``as_top_level_api``: ``init(particles)``, ``step(rng_key,
    state)``; at most ``max_iterations`` steps."""
    if int(max_iterations) < 1:
        raise ValueError(f"max_iterations must be at least 1, got {max_iterations}")
    kernel = build_kernel(logprior_fn, loglikelihood_fn, mcmc_step_fn, mcmc_init_fn, resampling_fn, target_ess,
                          root_solver)
    loglikelihood = kernel.tempered_logdensity.loglikelihood

    def init_fn(particles, rng_key=None):
        del rng_key
        return init(particles, loglikelihood, max_iterations)

    def step_fn(rng_key, state):
        return kernel(rng_key, state, num_mcmc_steps, mcmc_parameters)

    return SamplingAlgorithm(init_fn, step_fn)
