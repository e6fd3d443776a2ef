"""Sequential Monte Carlo behind ``blackjax.smc``: tempered, adaptive tempered, persistent-sampling and adaptive
persistent-sampling SMC whose particles are the ``(N, D)`` chain batch of this package and whose move is
``num_mcmc_steps`` transitions of its own samplers -- or, waste-free, ``p - 1`` transitions of ``N / p`` of them with
every state kept -- optionally re-tuned from the particles after every temperature, or pretuned: a population of
move parameters, one value per particle, adapted before every step.

Modules mirror the reference: ``base``, ``resampling``, ``ess``, ``solver``, ``tempered``, ``adaptive_tempered``,
``persistent_sampling``, ``adaptive_persistent_sampling``, ``waste_free``, ``inner_kernel_tuning``, ``pretuning``,
``tuning``.
Out of scope: partial-posteriors, waste-free moves inside persistent sampling, pytrees of particles, particles sharded
across GPUs.
"""
from . import (adaptive_persistent_sampling, adaptive_tempered, base, ess, inner_kernel_tuning, persistent_sampling,
               pretuning, resampling, solver, tempered, tuning, waste_free)
from .base import extend_params
from .waste_free import waste_free_smc

__all__ = ["adaptive_persistent_sampling", "adaptive_tempered", "base", "ess", "inner_kernel_tuning",
           "persistent_sampling", "pretuning", "resampling", "solver", "tempered", "tuning", "waste_free",
           "extend_params", "waste_free_smc"]
