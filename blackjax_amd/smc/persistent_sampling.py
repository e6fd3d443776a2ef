"""Persistent-sampling SMC on MI355X behind the ``blackjax.persistent_sampling_smc`` API surface.

Mirrors blackjax/smc/persistent_sampling.py (Karamanis & Seljak 2024): ``PersistentSMCState``,
``PersistentStateInfo``, ``init``, ``remove_padding``, ``compute_log_Z``, ``compute_log_persistent_weights``,
``resample_from_persistent``, ``step``, ``build_kernel`` and ``as_top_level_api``.  The sampler keeps the particles of
EVERY iteration.  The step to iteration ``i`` at temperature ``lam`` (smc/persistent_sampling.py::step) weighs the
``P = i * N`` particles of slots ``s < i`` against the mixture of the tempered targets they were drawn from:

1. ``updating_key, resampling_key = split(rng_key, 2)``;
2. ``den_j = logsumexp_{s<i}(lambda_s * ll_j - logZ_s) - log(i)`` (``bjx_smc_persistent_denominator``),
   ``lw_j = lam * ll_j - den_j``, ``logZ_i = logsumexp(lw) - log(P)``, ``W = exp(lw - logsumexp(lw))``
   (``bjx_smc_persistent_weights``: tile partials in fp64 over the whole device, combined by a later launch);
3. ``N`` ancestors in ``[0, P)`` from ``W``, rows gathered from the flat ``(P, D)`` view of the persistent particles;
4. ``num_mcmc_steps`` transitions of ``mcmc_step_fn`` on ``logprior + lam * loglikelihood`` -- the NEW temperature,
   unlike ``blackjax_amd.smc.tempered`` -- particle ``k`` keyed ``split(split(updating_key, N)[k], num_mcmc_steps)[m]``;
5. slot ``i`` receives the moved particles, their log-likelihoods, ``logZ_i`` and ``lam``.

The log evidence is ``state.log_Z`` itself (``persistent_log_Z[iteration]``), not a sum of increments, and estimates
under ``state.persistent_weights`` use all ``(iteration + 1) * N`` particles.  At ``i = 1`` the arithmetic is the
tempered step's: ``den = 0``, ``lw = lam * ll``, ``logZ_1 = log mean exp``.

Deliberate differences from the reference:

* ``lambda_s * ll`` is exactly 0 when ``lambda_s == 0`` whatever ``ll`` is (the weighting rule of ``csrc/bjx_smc_dev.h``), and a
  NaN or ``-inf`` log-weight is a particle of weight 0 that takes no part in any sum.  If no particle counts the
  weights are NaN and ``logZ_i = -inf``; no host check is made for it.
* ``iteration`` is a Python int (the step count is known on the host), so nothing is read back from the device.
* The slots are written IN PLACE: all states of one run share their buffers.  An earlier state stays valid for its own
  ``iteration`` because no slot beyond it is ever read.
* A step beyond ``n_schedule`` raises ``ValueError``, and ``init`` checks ``(n_schedule + 1) * N <= 2**24``
  (resampling positions are fp32).

Out of scope: as for ``blackjax_amd.smc.tempered``, waste-free moves (``smc.waste_free`` is not supported here: the
step always resamples ``N``) and inner-kernel tuning around this sampler, and updating ``den`` incrementally from one
step to the next.
"""
from __future__ import annotations

import math
from typing import Callable, NamedTuple

import torch

from .. import _lib
from .._util import check_batch
from ..base import SamplingAlgorithm
from ..random import split
from . import base
from .resampling import MAX_PARTICLES
from .tempered import TemperedLogDensity

__all__ = ["PersistentSMCState", "PersistentStateInfo", "REDUCTION_TILE", "init", "remove_padding", "compute_log_Z",
           "compute_log_persistent_weights", "compute_persistent_weights", "resample_from_persistent", "step",
           "build_kernel", "as_top_level_api"]

REDUCTION_TILE = 1024  # particles per workgroup of the grid-wide reductions (bjx_smc_persistent_tile())


class PersistentSMCState(NamedTuple):
    """blackjax/smc/persistent_sampling.py ``PersistentSMCState``: slots ``0 .. n_schedule`` filled up to
    ``iteration``, zero beyond it.  ``persistent_particles`` (T+1, N, D), ``persistent_log_likelihoods`` (T+1, N),
    ``persistent_log_Z`` (T+1,), ``tempering_schedule`` (T+1,): float32 device tensors; ``iteration``: a Python int."""

    persistent_particles: torch.Tensor
    persistent_log_likelihoods: torch.Tensor
    persistent_log_Z: torch.Tensor
    tempering_schedule: torch.Tensor
    iteration: int

    @property
    def particles(self) -> torch.Tensor:
        """(N, D): the particles of the current iteration (a view)."""
        return self.persistent_particles[self.iteration]

    @property
    def log_likelihoods(self) -> torch.Tensor:
        return self.persistent_log_likelihoods[self.iteration]

    @property
    def log_Z(self) -> torch.Tensor:
        """0-d: the log evidence estimate at the current temperature."""
        return self.persistent_log_Z[self.iteration]

    @property
    def tempering_param(self) -> torch.Tensor:
        return self.tempering_schedule[self.iteration]

    @property
    def n_particles(self) -> int:
        return int(self.persistent_particles.shape[1])

    @property
    def persistent_weights(self) -> torch.Tensor:
        """(T+1, N) weights of all particles up to and including the current iteration, mean 1 over the live rows
        and 0 beyond them (smc/persistent_sampling.py::compute_persistent_weights with ``include_current=True``)."""
        return compute_persistent_weights(self.persistent_log_likelihoods, self.persistent_log_Z,
                                          self.tempering_schedule, self.iteration, include_current=True)[0]


class PersistentStateInfo(NamedTuple):
    """blackjax/smc/persistent_sampling.py ``PersistentStateInfo``: (N,) int32 ancestors in ``[0, i * N)``, the
    update's info."""

    ancestors: torch.Tensor
    update_info: object


def init(particles, loglikelihood_fn: Callable, n_schedule: int) -> PersistentSMCState:
    """blackjax/smc/persistent_sampling.py ``init``: slot 0 holds the particles and their log-likelihoods,
    ``lambda_0 = 0`` and ``logZ_0 = 0``.  ``loglikelihood_fn``: (N, D) -> (N,)."""
    x = base.check_particles(particles)
    n_schedule = int(n_schedule)
    if n_schedule < 1:
        raise ValueError(f"n_schedule must be at least 1, got {n_schedule}")
    n, d = x.shape
    if (n_schedule + 1) * n > MAX_PARTICLES:
        raise ValueError(f"(n_schedule + 1) * n_particles must not exceed 2**24 (resampling positions are fp32), got "
                         f"{n_schedule + 1} * {n}")
    ll = loglikelihood_fn(x)
    if ll.shape != (n,):
        raise ValueError(f"loglikelihood_fn must return ({n},), got {tuple(ll.shape)}")
    pp = torch.zeros((n_schedule + 1, n, d), dtype=torch.float32, device=x.device)
    pll = torch.zeros((n_schedule + 1, n), dtype=torch.float32, device=x.device)
    pp[0].copy_(x)
    pll[0].copy_(ll.detach())
    return PersistentSMCState(pp, pll, torch.zeros(n_schedule + 1, dtype=torch.float32, device=x.device),
                              torch.zeros(n_schedule + 1, dtype=torch.float32, device=x.device), 0)


def remove_padding(state: PersistentSMCState) -> PersistentSMCState:
    """blackjax/smc/persistent_sampling.py ``remove_padding``: the live slots ``0 .. iteration`` only (views)."""
    k = state.iteration + 1
    return PersistentSMCState(state.persistent_particles[:k], state.persistent_log_likelihoods[:k],
                              state.persistent_log_Z[:k], state.tempering_schedule[:k], state.iteration)


def _check_persistent(persistent_log_likelihoods, persistent_log_Z, tempering_schedule, iteration, include_current):
    pll = check_batch(persistent_log_likelihoods, "persistent_log_likelihoods")
    if pll.ndim != 2 or pll.shape[1] < 1:
        raise ValueError(f"persistent_log_likelihoods must be (n_slots, n_particles), got {tuple(pll.shape)}")
    plz = check_batch(persistent_log_Z, "persistent_log_Z")
    sched = check_batch(tempering_schedule, "tempering_schedule")
    slots = pll.shape[0]
    if plz.shape != (slots,) or sched.shape != (slots,):
        raise ValueError(f"persistent_log_Z and tempering_schedule must be ({slots},), got {tuple(plz.shape)} and "
                         f"{tuple(sched.shape)}")
    iteration = int(iteration)
    n_terms = iteration + (1 if include_current else 0)
    if not (0 <= iteration < slots and n_terms >= 1):
        raise ValueError(f"iteration {iteration} (include_current={bool(include_current)}) does not fit {slots} slots")
    if n_terms * pll.shape[1] > MAX_PARTICLES:
        raise ValueError("the persistent set must not exceed 2**24 particles (resampling positions are fp32)")
    return pll, plz, sched, iteration, n_terms


def _workspace(P: int, device) -> torch.Tensor:
    return torch.empty(_lib.load().bjx_smc_persistent_workspace_bytes(P) // 8, dtype=torch.float64, device=device)


def _denominator(pll, plz, sched, n_terms: int) -> torch.Tensor:
    """(P,) mixture denominators of the rows of slots ``s < n_terms``."""
    P = n_terms * pll.shape[1]
    den = torch.empty(P, dtype=torch.float32, device=pll.device)
    _lib.call("bjx_smc_persistent_denominator", _lib.current_stream(), P, n_terms, pll.data_ptr(), sched.data_ptr(),
              plz.data_ptr(), den.data_ptr())
    return den


def _weigh(pll, plz, sched, iteration: int, n_terms: int, want_log: bool, want_weights: bool):
    """-> (normalised log-weights (P,) or None, normalised weights (P,) or None, log_Z 0-d) at the temperature of slot
    ``iteration`` over the rows of slots ``s < n_terms``."""
    P = n_terms * pll.shape[1]
    dev = pll.device
    den = _denominator(pll, plz, sched, n_terms)
    lw = torch.empty(P, dtype=torch.float32, device=dev) if want_log else None
    w = torch.empty(P, dtype=torch.float32, device=dev) if want_weights else None
    log_z = torch.empty((), dtype=torch.float32, device=dev)
    _lib.call("bjx_smc_persistent_weights", _lib.current_stream(), P, pll.data_ptr(), den.data_ptr(),
              sched.data_ptr() + 4 * iteration, _workspace(P, dev).data_ptr(), _lib.ptr(lw), _lib.ptr(w),
              log_z.data_ptr())
    return lw, w, log_z


def _padded(flat: torch.Tensor, shape, fill: float) -> torch.Tensor:
    out = torch.full(shape, fill, dtype=torch.float32, device=flat.device)
    out.view(-1)[: flat.shape[0]].copy_(flat)
    return out


def compute_log_persistent_weights(persistent_log_likelihoods, persistent_log_Z, tempering_schedule, iteration,
                                   include_current: bool = False, normalize_to_one: bool = False):
    """blackjax/smc/persistent_sampling.py ``compute_log_persistent_weights``: ``(log_weights (T+1, N), log_Z)`` at
    the temperature ``tempering_schedule[iteration]`` over the slots ``s < iteration`` (``s <= iteration`` with
    ``include_current``); slots beyond them are ``-inf``.  The log-weights are shifted by their log-sum-exp when
    ``normalize_to_one`` (they sum to 1), by ``log_Z`` otherwise (their mean is 1)."""
    pll, plz, sched, iteration, n_terms = _check_persistent(persistent_log_likelihoods, persistent_log_Z,
                                                            tempering_schedule, iteration, include_current)
    lw, _, log_z = _weigh(pll, plz, sched, iteration, n_terms, True, False)
    if not normalize_to_one:
        lw = lw + math.log(n_terms * pll.shape[1])
    return _padded(lw, pll.shape, -math.inf), log_z


def compute_persistent_weights(persistent_log_likelihoods, persistent_log_Z, tempering_schedule, iteration,
                               include_current: bool = False, normalize_to_one: bool = False):
    """blackjax/smc/persistent_sampling.py ``compute_persistent_weights``: ``(weights (T+1, N), log_Z)``, the
    exponential of ``compute_log_persistent_weights`` taken in fp64 by the kernel; 0 beyond the live slots."""
    pll, plz, sched, iteration, n_terms = _check_persistent(persistent_log_likelihoods, persistent_log_Z,
                                                            tempering_schedule, iteration, include_current)
    _, w, log_z = _weigh(pll, plz, sched, iteration, n_terms, False, True)
    if not normalize_to_one:
        w = w * float(n_terms * pll.shape[1])
    return _padded(w, pll.shape, 0.0), log_z


def compute_log_Z(log_weights, iteration) -> torch.Tensor:
    """blackjax/smc/persistent_sampling.py ``compute_log_Z``: ``logsumexp(log_weights) - log(iteration * N)`` of
    UNNORMALISED log-weights ``(T+1, N)`` whose slots beyond the live ones are ``-inf`` (``bjx_smc_reweight``'s
    fp64 log-sum-exp).  The step itself takes ``log_Z`` from ``bjx_smc_persistent_weights``."""
    lw = check_batch(log_weights, "log_weights")
    if lw.ndim != 2:
        raise ValueError(f"log_weights must be (n_slots, n_particles), got {tuple(lw.shape)}")
    flat = lw.reshape(-1)
    _, inc = base.normalize(flat)  # logsumexp - log(numel)
    return inc + (math.log(flat.shape[0]) - math.log(int(iteration) * lw.shape[1]))


def resample_from_persistent(rng_key, persistent_particles, persistent_weights, resample_fn: Callable):
    """blackjax/smc/persistent_sampling.py ``resample_from_persistent``: ``N`` rows of the flat view of the
    ``(S, N, D)`` persistent particles drawn with the ``(S, N)`` weights (normalised to sum to 1) -> (particles (N, D),
    ancestors (N,) int32 in ``[0, S * N)``)."""
    pp = check_batch(persistent_particles, "persistent_particles")
    if pp.ndim != 3:
        raise ValueError(f"persistent_particles must be (n_slots, n_particles, dim), got {tuple(pp.shape)}")
    w = check_batch(persistent_weights, "persistent_weights")
    if w.shape != pp.shape[:2]:
        raise ValueError(f"persistent_weights must be {tuple(pp.shape[:2])}, got {tuple(w.shape)}")
    ancestors = resample_fn(rng_key, w.reshape(-1), pp.shape[1])
    return base.gather(pp.reshape(-1, pp.shape[2]), ancestors), ancestors


def _check_state(state: PersistentSMCState):
    pp = check_batch(state.persistent_particles, "state.persistent_particles")
    if pp.ndim != 3:
        raise ValueError(f"state.persistent_particles must be (n_slots, n_particles, dim), got {tuple(pp.shape)}")
    pll = check_batch(state.persistent_log_likelihoods, "state.persistent_log_likelihoods")
    if pll.shape != pp.shape[:2]:
        raise ValueError(f"state.persistent_log_likelihoods must be {tuple(pp.shape[:2])}, got {tuple(pll.shape)}")
    return pp, pll


def step(rng_key, state: PersistentSMCState, lmbda, loglikelihood_fn: Callable, update_fn: Callable,
         resample_fn: Callable, weight_fn: Callable = compute_log_persistent_weights):
    """blackjax/smc/persistent_sampling.py ``step``: one iteration at temperature ``lmbda`` (a number or a 0-d
    tensor).  ``update_fn(rng_key, particles) -> (particles, info)`` moves the resampled particles,
    ``loglikelihood_fn`` maps (N, D) to (N,), ``weight_fn`` has the signature of ``compute_log_persistent_weights``.
    Slot ``iteration + 1`` of the state's buffers is written in place."""
    pp, pll = _check_state(state)
    slots, n, d = pp.shape
    i = int(state.iteration) + 1
    if i >= slots:
        raise ValueError(f"the state holds {slots - 1} iterations (n_schedule) and all of them are taken")
    plz, sched = state.persistent_log_Z, state.tempering_schedule
    sched[i].copy_(base.device_scalar(lmbda, pp.device))
    keys = split(rng_key, 2)
    updating_key, resampling_key = keys[0], keys[1]
    if weight_fn is compute_log_persistent_weights:  # the kernel's own fp64 exponential
        _, weights, log_z = _weigh(pll, plz, sched, i, i, False, True)
    else:
        log_w, log_z = weight_fn(pll, plz, sched, i, include_current=False, normalize_to_one=True)
        weights = torch.exp(log_w.reshape(-1)[: i * n])
    ancestors = getattr(resample_fn, "_bjx_trusted", resample_fn)(resampling_key, weights, n)
    x = base.gather(pp.view(slots * n, d)[: i * n], ancestors)
    x, update_info = update_fn(updating_key, x)
    pp[i].copy_(x)
    pll[i].copy_(loglikelihood_fn(x).detach())
    plz[i].copy_(log_z)
    return (PersistentSMCState(pp, pll, plz, sched, i), PersistentStateInfo(ancestors, update_info))


def build_kernel(logprior_fn: Callable, loglikelihood_fn: Callable, mcmc_step_fn: Callable, mcmc_init_fn: Callable,
                 resampling_fn: Callable, update_strategy: Callable = base.update_and_take_last):
    """blackjax/smc/persistent_sampling.py ``build_kernel``: ``kernel(rng_key, state, num_mcmc_steps, lmbda,
    mcmc_parameters)``.  The arguments are those of ``blackjax_amd.smc.tempered.build_kernel``; the move targets the
    NEW temperature through the algorithm's one ``TemperedLogDensity``."""
    tempered = TemperedLogDensity(logprior_fn, loglikelihood_fn)

    def kernel(rng_key, state: PersistentSMCState, num_mcmc_steps: int, lmbda, mcmc_parameters: dict):
        n = state.persistent_particles.shape[1]
        lam_new = base.device_scalar(lmbda, state.persistent_particles.device)

        def update_fn(key, x):
            tempered.set_temperature(lam_new)
            update, _ = update_strategy(mcmc_init_fn, tempered, mcmc_step_fn, num_mcmc_steps, n)
            return update(key, x, mcmc_parameters)

        return step(rng_key, state, lam_new, tempered.loglikelihood, update_fn, resampling_fn)

    kernel.tempered_logdensity = tempered
    return kernel


def as_top_level_api(logprior_fn: Callable, loglikelihood_fn: Callable, n_schedule: int, mcmc_step_fn: Callable,
                     mcmc_init_fn: Callable, mcmc_parameters: dict, resampling_fn: Callable,
                     num_mcmc_steps: int = 10) -> SamplingAlgorithm:
    """blackjax/smc/persistent_sampling.py ``as_top_level_api``: ``init(particles)``, ``step(rng_key, state,
    lmbda)``; at most ``n_schedule`` steps."""
    if int(n_schedule) < 1:
        raise ValueError(f"n_schedule must be at least 1, got {n_schedule}")
    kernel = build_kernel(logprior_fn, loglikelihood_fn, mcmc_step_fn, mcmc_init_fn, resampling_fn)
    loglikelihood = kernel.tempered_logdensity.loglikelihood

    def init_fn(particles, rng_key=None):
        del rng_key
        return init(particles, loglikelihood, n_schedule)

    def step_fn(rng_key, state, lmbda):
        return kernel(rng_key, state, num_mcmc_steps, lmbda, mcmc_parameters)

    return SamplingAlgorithm(init_fn, step_fn)
