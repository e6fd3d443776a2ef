"""Root solver of the adaptive temperature behind ``blackjax.smc.solver``.

Mirrors blackjax/smc/solver.py ``dichotomy``, specialised to the one function the package solves,
``f(delta) = log_ess(delta * loglikelihood) - log(N * target_ess)``: the whole bisection is one launch
(``bjx_smc_ess_solve``, include/bjx_hip.h "SMC") and returns a device scalar, so no iteration of it makes a host
round trip.  Other root solvers of the reference are out of scope.
"""
from __future__ import annotations

import torch

from .. import _lib
from .._util import check_batch
from .base import device_scalar

__all__ = ["dichotomy", "next_temperature"]


def _check(loglikelihood, target_ess):
    ll = check_batch(loglikelihood, "loglikelihood")
    if ll.ndim != 1 or ll.shape[0] < 1:
        raise ValueError(f"loglikelihood must be (n_particles,), got {tuple(ll.shape)}")
    target_ess = float(target_ess)
    if not 0.0 < target_ess <= 1.0:
        raise ValueError(f"target_ess is a fraction of the particles in (0, 1], got {target_ess}")
    return ll, target_ess


def dichotomy(loglikelihood, target_ess, max_delta) -> torch.Tensor:
    """The largest ``delta`` in ``[0, max_delta]`` whose ESS is at least ``target_ess * N``: ``max_delta`` itself
    if its ESS is, else 30 halvings in fp32 that keep the ESS at the left end at or above the target and return the
    left end.  ``loglikelihood``: ``(N,)`` device tensor; ``max_delta``: a number or a 0-d tensor; returns a 0-d
    device tensor."""
    ll, target_ess = _check(loglikelihood, target_ess)
    md = device_scalar(max_delta, ll.device)
    delta = torch.empty((), dtype=torch.float32, device=ll.device)
    _lib.call("bjx_smc_ess_solve", _lib.current_stream(), ll.shape[0], ll.data_ptr(), target_ess, md.data_ptr(), None,
              delta.data_ptr(), None)
    return delta


def next_temperature(loglikelihood, target_ess, lmbda):
    """``dichotomy`` on ``[0, 1 - lmbda]`` fused with the temperature update: ``(delta, lmbda + delta)``, the new
    temperature being exactly 1.0 when the whole remaining interval is taken."""
    ll, target_ess = _check(loglikelihood, target_ess)
    lam = device_scalar(lmbda, ll.device)
    delta = torch.empty((), dtype=torch.float32, device=ll.device)
    lam_new = torch.empty((), dtype=torch.float32, device=ll.device)
    _lib.call("bjx_smc_ess_solve", _lib.current_stream(), ll.shape[0], ll.data_ptr(), target_ess, None, lam.data_ptr(),
              delta.data_ptr(), lam_new.data_ptr())
    return delta, lam_new
