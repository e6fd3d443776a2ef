"""Stochastic-gradient MCMC behind ``blackjax.sgmcmc``: ``sgld``, ``sghmc`` and ``sgnht`` over the ``(N, D)`` chain
batch of this package, for models whose gradient is estimated on a minibatch that changes every step.

Modules mirror the reference: ``sgld``, ``sghmc``, ``sgnht``, ``diffusions``, ``gradients``.  The user side of a step
is one autograd pass (``grad_estimator(position, minibatch) -> (N, D)``, never traced); the noise draw, the diffusion
update and the thermostat are one HIP launch per step.  Out of scope: ``csgld``.
"""
from . import diffusions, gradients, sghmc, sgld, sgnht
from .gradients import control_variates, grad_estimator, logdensity_estimator

__all__ = ["diffusions", "gradients", "sghmc", "sgld", "sgnht", "control_variates", "grad_estimator",
           "logdensity_estimator"]
