"""Inner-kernel tuning behind ``blackjax.inner_kernel_tuning``: tempered SMC whose move is re-tuned from the
particles (or from the move's own info) after every temperature.

Mirrors blackjax/smc/inner_kernel_tuning.py: ``StateWithParameterOverride``, ``init``, ``build_kernel`` and
``as_top_level_api``.  One step:

1. ``parameter_update_key, step_key = split(rng_key, 2)``;
2. the inner SMC algorithm steps with ``mcmc_parameters = state.parameter_override``, keyed ``step_key``;
3. ``new_override = mcmc_parameter_update_fn(parameter_update_key, new_state, info)``.

The reference constructs ``smc_algorithm(...)`` anew at every step.  Here that would rebuild the tempered
log-density and trace both user callables once per temperature, so the inner kernel is built ONCE through
``smc_algorithm.build_kernel`` and every step hands it the current override as its ``mcmc_parameters`` argument:
``kernel.tempered_logdensity`` is one object for the life of the kernel.  ``smc_algorithm`` is
``blackjax_amd.tempered_smc`` or ``blackjax_amd.adaptive_tempered_smc``; ``extra_parameters`` passes ``target_ess``,
``root_solver`` and ``update_strategy`` through to it.  The override is a dict of keyword arguments of the move, as
``mcmc_parameters`` is everywhere in ``blackjax_amd.smc``; nothing in a step is read back by the host.

Out of scope: partial posteriors.  Parameters kept per particle and adapted BEFORE a step are
``blackjax_amd.smc.pretuning``.
"""
from __future__ import annotations

from typing import Callable, NamedTuple

from ..base import SamplingAlgorithm
from ..random import split
from . import adaptive_tempered, tempered

__all__ = ["StateWithParameterOverride", "init", "build_kernel", "as_top_level_api"]


class StateWithParameterOverride(NamedTuple):
    """blackjax/smc/inner_kernel_tuning.py ``StateWithParameterOverride``: the inner algorithm's state and the
    ``mcmc_parameters`` its next step will use."""

    sampler_state: object
    parameter_override: object


def init(alg_init_fn: Callable, position, initial_parameter_value) -> StateWithParameterOverride:
    """blackjax/smc/inner_kernel_tuning.py ``init``."""
    return StateWithParameterOverride(alg_init_fn(position), initial_parameter_value)


def _inner_build_kernel(smc_algorithm, wrapper: str = "inner_kernel_tuning") -> tuple[Callable, bool]:
    """-> (the ``build_kernel`` of the algorithm, whether it is the adaptive one); ``wrapper`` names the caller in the
    error (``smc.pretuning`` resolves its inner algorithm here too)."""
    build = getattr(smc_algorithm, "build_kernel", None)
    if build is tempered.build_kernel:
        return build, False
    if build is adaptive_tempered.build_kernel:
        return build, True
    raise TypeError(f"{wrapper} wraps blackjax_amd.tempered_smc or blackjax_amd.adaptive_tempered_smc, got "
                    f"{smc_algorithm!r}")


def build_kernel(smc_algorithm, logprior_fn: Callable, loglikelihood_fn: Callable, mcmc_step_fn: Callable,
                 mcmc_init_fn: Callable, resampling_fn: Callable, mcmc_parameter_update_fn: Callable,
                 num_mcmc_steps: int = 10, **extra_parameters) -> Callable:
    """blackjax/smc/inner_kernel_tuning.py ``build_kernel``: ``kernel(rng_key, state, **extra_step_parameters) ->
    (StateWithParameterOverride, info)``; ``extra_step_parameters`` is ``lmbda=`` for ``tempered_smc`` and empty for
    ``adaptive_tempered_smc``.  ``mcmc_parameter_update_fn(rng_key, new_inner_state, info) -> mcmc_parameters``."""
    build, adaptive = _inner_build_kernel(smc_algorithm)
    allowed = {"target_ess", "root_solver", "update_strategy"} if adaptive else {"update_strategy"}
    unknown = set(extra_parameters) - allowed
    if unknown:
        raise TypeError(f"unexpected extra parameters {sorted(unknown)}: the inner algorithm takes {sorted(allowed)}")
    if adaptive and "target_ess" not in extra_parameters:
        raise TypeError("adaptive_tempered_smc needs target_ess=")
    inner = build(logprior_fn, loglikelihood_fn, mcmc_step_fn, mcmc_init_fn, resampling_fn, **extra_parameters)

    def kernel(rng_key, state: StateWithParameterOverride, **extra_step_parameters):
        keys = split(rng_key, 2)
        parameter_update_key, step_key = keys[0], keys[1]
        if adaptive:
            new_state, info = inner(step_key, state.sampler_state, num_mcmc_steps, state.parameter_override,
                                    **extra_step_parameters)
        else:
            if "lmbda" not in extra_step_parameters:
                raise TypeError("a step of tempered_smc needs lmbda=")
            lmbda = extra_step_parameters.pop("lmbda")
            new_state, info = inner(step_key, state.sampler_state, num_mcmc_steps, lmbda, state.parameter_override,
                                    **extra_step_parameters)
        new_override = mcmc_parameter_update_fn(parameter_update_key, new_state, info)
        return StateWithParameterOverride(new_state, new_override), info

    kernel.tempered_logdensity = inner.tempered_logdensity
    return kernel


def as_top_level_api(smc_algorithm, logprior_fn: Callable, loglikelihood_fn: Callable, mcmc_step_fn: Callable,
                     mcmc_init_fn: Callable, resampling_fn: Callable, mcmc_parameter_update_fn: Callable,
                     initial_parameter_value, num_mcmc_steps: int = 10, **extra_parameters) -> SamplingAlgorithm:
    """blackjax/smc/inner_kernel_tuning.py ``as_top_level_api``: ``init(position)``, ``step(rng_key, state,
    **extra_step_parameters)``."""
    kernel = build_kernel(smc_algorithm, logprior_fn, loglikelihood_fn, mcmc_step_fn, mcmc_init_fn, resampling_fn,
                          mcmc_parameter_update_fn, num_mcmc_steps, **extra_parameters)

    def init_fn(position, rng_key=None):
        del rng_key
        return init(smc_algorithm.init, position, initial_parameter_value)

    def step_fn(rng_key, state, **extra_step_parameters):
        return kernel(rng_key, state, **extra_step_parameters)

    return SamplingAlgorithm(init_fn, step_fn)
