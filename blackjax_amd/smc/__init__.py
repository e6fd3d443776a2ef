"""Sequential Monte Carlo behind ``blackjax.smc``: tempered, adaptive tempered, persistent-sampling and adaptive
persistent-sampling SMC whose particles are the ``(N, D)`` chain batch of this package and whose move is
``num_mcmc_steps`` transitions of its own samplers.

Modules mirror the reference: ``base``, ``resampling``, ``ess``, ``solver``, ``tempered``, ``adaptive_tempered``,
``persistent_sampling``, ``adaptive_persistent_sampling``.
Out of scope: ``multinomial`` / ``residual`` resampling, partial-posteriors, pretuning and waste-free SMC,
inner-kernel tuning, pytrees of particles, particles sharded across GPUs.
"""
from . import (adaptive_persistent_sampling, adaptive_tempered, base, ess, persistent_sampling, resampling, solver,
               tempered)
from .base import extend_params

__all__ = ["adaptive_persistent_sampling", "adaptive_tempered", "base", "ess", "persistent_sampling", "resampling",
           "solver", "tempered", "extend_params"]
