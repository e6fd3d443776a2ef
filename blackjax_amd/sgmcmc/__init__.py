"""Stochastic-gradient MCMC behind ``blackjax.sgmcmc``: ``sgld``, ``sghmc``, ``sgnht`` and ``csgld`` over the
``(N, D)`` chain batch of this package, for models whose gradient is estimated on a minibatch that changes every step.

Modules mirror the reference: ``sgld``, ``sghmc``, ``sgnht``, ``csgld``, ``diffusions``, ``gradients``.  The user side
of a step is one autograd pass (``grad_estimator(position, minibatch) -> (N, D)``, never traced); the noise draw, the
diffusion update and the thermostat are one HIP launch per step.  ``csgld`` (contour SGLD, the multimodal member) also
calls ``logdensity_estimator(position, minibatch) -> (N,)`` at the new position and keeps a per-chain energy
histogram: two launches per step, the scaled-gradient Langevin update and the histogram update.
"""
from . import csgld, diffusions, gradients, sghmc, sgld, sgnht
from .gradients import control_variates, grad_estimator, logdensity_estimator

__all__ = ["csgld", "diffusions", "gradients", "sghmc", "sgld", "sgnht", "control_variates", "grad_estimator",
           "logdensity_estimator"]
