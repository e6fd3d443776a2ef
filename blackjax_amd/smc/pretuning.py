"""Pretuning behind ``blackjax.pretuning``: tempered SMC that carries a population of move parameters, one value per
particle, and adapts it before every step (Fearnhead & Taylor 2013, "An adaptive sequential Monte Carlo sampler",
eq. 4).

Mirrors blackjax/smc/pretuning.py: ``SMCInfoWithParameterDistribution``, ``esjd``, ``update_parameter_distribution``,
``default_measure_factory``, ``build_pretune``, ``init``, ``build_kernel`` and ``as_top_level_api``.  One step:

1. ``step_key, pretune_key = split(rng_key, 2)``;
2. the pretune: ONE trial transition of all ``N`` particles at the state's temperature, particle ``i`` with its own
   parameters (row ``i`` of every sampled entry of the override); each parameter row is scored by the expected
   squared jump distance of its particle, ``acceptance_rate * |previous - next|^2`` in the move's metric
   (``bjx_smc_esjd``); the weights are ``alpha + measure`` normalised (``bjx_smc_pretune_weights``); ancestors are
   drawn from them and every sampled entry becomes ``jitter(P)[ancestors]`` (``bjx_smc_jitter_gather``);
3. the inner SMC algorithm steps with ``mcmc_parameters`` = the new override, keyed ``step_key``.

Where ``inner_kernel_tuning`` gives all particles one parameter set re-estimated AFTER a step, pretuning keeps a
distribution of them and updates it BEFORE the step.  The sampled parameters are the keys of ``sigma_parameters``:
``(N,)`` or ``(N, K)`` float32 device tensors in the override; every other entry of the override is shared by all
particles and is handed on untouched (the same object).  As in ``inner_kernel_tuning`` the inner kernel is built
ONCE; nothing in a step is read back by the host and nothing is traced per step.

Deliberate deviations from the reference.  The ancestors of the parameter rows are drawn with this package's
multinomial resampling (``smc.resampling.multinomial``) where the reference calls ``jax.random.choice(p=weights)``:
the same distribution, reproducible bit for bit.  ``positive_parameters`` names sampled entries that are jittered
multiplicatively, ``p * exp(sigma * z)``, so that a step size or an inverse mass stays positive; every other sampled
entry gets additive noise, ``p + sigma * z``.  A trial whose measure is NaN, infinite or negative scores 0: its
parameters weigh ``alpha``.
"""
from __future__ import annotations

import sys
from typing import Callable, NamedTuple

import torch

from .. import _lib, metrics
from .._util import check_batch
from ..base import SamplingAlgorithm
from ..random import key_words, split
from . import base, resampling
from .inner_kernel_tuning import StateWithParameterOverride, _inner_build_kernel
from .inner_kernel_tuning import init  # blackjax/smc/pretuning.py ``init`` is the same function: inner state + override

__all__ = ["SMCInfoWithParameterDistribution", "StateWithParameterOverride", "esjd", "update_parameter_distribution",
           "default_measure_factory", "build_pretune", "init", "build_kernel", "as_top_level_api", "pretune_weights",
           "jitter_gather"]

MAX_COLUMNS = 1 << 20


class SMCInfoWithParameterDistribution(NamedTuple):
    """blackjax/smc/pretuning.py ``SMCInfoWithParameterDistribution``: the inner step's info and the parameters the
    step was made with."""

    smc_info: object
    parameter_override: object


def _rows(x, name: str, n=None) -> torch.Tensor:
    x = check_batch(x, name)
    if x.ndim != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{name} must be (n_particles, dim), got {tuple(x.shape)}")
    if n is not None and x.shape[0] != n:
        raise ValueError(f"{name} must have {n} rows, got {tuple(x.shape)}")
    return x


_CHOLESKY_CACHE: dict = {}


def _cholesky(imm: torch.Tensor) -> torch.Tensor:
    """The lower factor of a shared dense matrix, once per distinct matrix; no status is read back."""
    key = (imm.data_ptr(), imm._version, tuple(imm.shape))
    hit = _CHOLESKY_CACHE.get(key)
    if hit is None:
        if len(_CHOLESKY_CACHE) > 8:
            _CHOLESKY_CACHE.clear()
        hit = _CHOLESKY_CACHE[key] = (torch.linalg.cholesky_ex(imm, check_errors=False)[0], imm)
    return hit[0]


def esjd(inverse_mass_matrix) -> Callable:
    """blackjax/smc/pretuning.py ``esjd``: ``measure(previous_position, next_position, acceptance_probability) ->
    (N,)``, the expected squared jump distance ``acceptance_probability * d^T M d`` with ``d = previous - next`` and
    ``M`` the inverse of ``inverse_mass_matrix``.  ``inverse_mass_matrix``: a diagonal ``(D,)``, one diagonal per
    particle ``(N, D)`` (``metrics.PerChainDiag`` / ``PerChainDiagTensor`` when ``N == D``), a dense ``(D, D)`` shared
    by all particles, or ``None`` for the identity.  The row sums are taken in fp64 (``bjx_smc_esjd``); a measure
    that is NaN, infinite or negative comes back as exactly 0.  The dense matrix is factorised once (the Cholesky
    factor of ``torch.linalg.cholesky_ex``, whose status is not read back: a matrix that is not positive definite
    scores 0 everywhere) and the difference whitened with one triangular solve."""

    def measure(previous_position, next_position, acceptance_probability) -> torch.Tensor:
        prev = _rows(previous_position, "previous_position")
        n, d = prev.shape
        nxt = _rows(next_position, "next_position", n)
        if nxt.shape != prev.shape:
            raise ValueError(f"next_position must be {tuple(prev.shape)}, got {tuple(nxt.shape)}")
        acc = check_batch(acceptance_probability, "acceptance_probability")
        if acc.shape != (n,):
            raise ValueError(f"acceptance_probability must have shape ({n},), got {tuple(acc.shape)}")
        if n > resampling.MAX_PARTICLES or d > MAX_COLUMNS:
            raise ValueError(f"esjd supports at most 2**24 particles of at most 2**20 coordinates, got {n} x {d}")
        imm, imm_stride = None, 0
        if inverse_mass_matrix is not None:
            metric = metrics.default_metric(inverse_mass_matrix, n, d, prev.device)
            if metric.kind == "diag":
                imm, imm_stride = metric.imm, metric.imm_stride
            elif metric.kind == "dense":
                # d^T imm^-1 d = |L^-1 d|^2: the whitened difference against zero, identity metric
                prev = torch.linalg.solve_triangular(_cholesky(metric.imm), (prev - nxt).t(), upper=False).t()
                prev, nxt = prev.contiguous(), torch.zeros_like(prev)
            else:
                raise ValueError("esjd takes a diagonal, per-particle diagonal or shared dense inverse_mass_matrix")
        out = torch.empty(n, dtype=torch.float32, device=prev.device)
        _lib.call("bjx_smc_esjd", _lib.current_stream(), n, d, prev.data_ptr(), nxt.data_ptr(), acc.data_ptr(),
                  _lib.ptr(imm), imm_stride, out.data_ptr())
        return out

    return measure


def pretune_weights(measure, alpha: float) -> torch.Tensor:
    """``(alpha + measure) / sum(alpha + measure)`` over ``(N,)``, fp64 sums rounded once
    (``bjx_smc_pretune_weights``); uniform when the sum is 0."""
    m = check_batch(measure, "measure")
    if m.ndim != 1 or not 1 <= m.shape[0] <= resampling.MAX_PARTICLES:
        raise ValueError(f"measure must be (n_particles,) with at most 2**24 particles, got {tuple(m.shape)}")
    alpha = _checked_alpha(alpha)
    w = torch.empty_like(m)
    _lib.call("bjx_smc_pretune_weights", _lib.current_stream(), m.shape[0], alpha, m.data_ptr(), w.data_ptr())
    return w


def _checked_alpha(alpha) -> float:
    alpha = float(alpha)
    if not 0.0 <= alpha < float("inf"):
        raise ValueError(f"alpha must be finite and non-negative, got {alpha}")
    return alpha


def _sigma_arg(sigma, k: int, device, name: str):
    """-> ((1,) or (K,) float32 device tensor, stride 0 or 1).  A Python number costs one fill launch; a host array
    is uploaded, so callers that step repeatedly keep the result (``build_pretune`` does)."""
    if isinstance(sigma, torch.Tensor) or hasattr(sigma, "__len__"):
        t = torch.as_tensor(sigma, dtype=torch.float32, device=device).contiguous()
        if t.ndim == 0:
            return t.reshape(1), 0
        if t.shape != (k,):
            raise ValueError(f"sigma_parameters[{name!r}] must be a scalar or have shape ({k},), got {tuple(t.shape)}")
        return t, 1
    return torch.full((1,), float(sigma), dtype=torch.float32, device=device), 0


def jitter_gather(noise_key, parameters, ancestors, sigma, log_space: bool = False, _name: str = "parameters"):
    """``jitter(parameters)[ancestors]`` out of place (``bjx_smc_jitter_gather``): ``parameters`` ``(N,)`` or
    ``(N, K)``, ``ancestors`` ``(M,)`` int32 -> ``(M,)`` or ``(M, K)``.  The noise is ``normal(noise_key, (N, K))``,
    regenerated at the source row; ``sigma`` a scalar or ``(K,)``; ``log_space`` jitters ``p * exp(sigma * z)``."""
    p = check_batch(parameters, _name)
    if p.ndim not in (1, 2) or p.shape[0] < 1 or p.numel() == 0:
        raise ValueError(f"{_name} must be (n_particles,) or (n_particles, K), got {tuple(p.shape)}")
    n, k = p.shape[0], (1 if p.ndim == 1 else p.shape[1])
    if not isinstance(ancestors, torch.Tensor) or ancestors.dtype != torch.int32 or ancestors.ndim != 1:
        raise ValueError("ancestors must be a 1-d int32 tensor")
    if ancestors.device != p.device:
        raise RuntimeError(f"ancestors lives on {ancestors.device}, {_name} on {p.device}")
    m = ancestors.shape[0]
    if not (n <= resampling.MAX_PARTICLES and 1 <= m <= resampling.MAX_PARTICLES and k <= MAX_COLUMNS):
        raise ValueError(f"jitter_gather supports at most 2**24 rows of at most 2**20 columns, got {n} -> {m} x {k}")
    sg, stride = _sigma_arg(sigma, k, p.device, _name)
    k0, k1 = key_words(noise_key)
    a = ancestors.contiguous()
    out = torch.empty((m,) + tuple(p.shape[1:]), dtype=torch.float32, device=p.device)
    _lib.call("bjx_smc_jitter_gather", _lib.current_stream(), k0, k1, n, m, k, p.data_ptr(), a.data_ptr(),
              sg.data_ptr(), stride, 1 if log_space else 0, out.data_ptr())
    return out


def update_parameter_distribution(key, previous_param_samples: dict, previous_particles, latest_particles,
                                  measure_of_chain_mixing: Callable, alpha: float, sigma_parameters: dict,
                                  acceptance_probability, positive_parameters=()):
    """blackjax/smc/pretuning.py ``update_parameter_distribution``: ``noise_key, resampling_key = split(key, 2)``;
    the measure of every particle's trial, the weights ``alpha + measure`` normalised, ``N`` ancestors drawn from
    them, and every entry of ``previous_param_samples`` jittered with ``sigma_parameters[name]`` and gathered by those
    ancestors -- each entry with the same ``noise_key`` over its own flat index space, as the reference's ``tree.map``
    draws them.  -> (new parameter samples, the measure ``(N,)``).

    Deliberate deviation: the ancestors are ``smc.resampling.multinomial``'s (sorted uniforms, integer prefix sums)
    where the reference draws ``jax.random.choice(resampling_key, N, (N,), p=weights)`` -- the same distribution,
    reproducible bit for bit, and non-decreasing.  ``positive_parameters``: names jittered as ``p * exp(sigma * z)``."""
    alpha = _checked_alpha(alpha)
    missing = set(previous_param_samples) - set(sigma_parameters)
    if missing:
        raise ValueError(f"sigma_parameters has no entry for {sorted(missing)}")
    x0 = _rows(previous_particles, "previous_particles")
    n = x0.shape[0]
    for name, p in previous_param_samples.items():
        _checked_sample(p, name, n)
    keys = split(key, 2)
    noise_key, resampling_key = keys[0], keys[1]
    measure = measure_of_chain_mixing(x0, latest_particles, acceptance_probability)
    weights = pretune_weights(measure, alpha)
    ancestors = resampling.multinomial._bjx_trusted(resampling_key, weights, n)
    new = {name: jitter_gather(noise_key, p, ancestors, sigma_parameters[name], name in positive_parameters, name)
           for name, p in previous_param_samples.items()}
    return new, measure


def _checked_sample(p, name: str, n: int) -> torch.Tensor:
    p = check_batch(p, f"parameter_override[{name!r}]")
    if p.ndim not in (1, 2) or p.shape[0] != n or p.numel() == 0:
        raise ValueError(f"parameter_override[{name!r}] is sampled per particle: it must be ({n},) or ({n}, K), got "
                         f"{tuple(p.shape)}")
    return p


def default_measure_factory(state: StateWithParameterOverride) -> Callable:
    """blackjax/smc/pretuning.py ``default_measure_factory``: ``esjd`` in the metric of the state's
    ``inverse_mass_matrix``, the identity when the move has none."""
    return esjd(state.parameter_override.get("inverse_mass_matrix"))


def _info_has_acceptance_rate(mcmc_step_fn):
    """Whether the info of a move of this package carries ``acceptance_rate``: read off the ``*Info`` tuples of the
    module that built the kernel.  None when that cannot be told without running it."""
    fn = getattr(mcmc_step_fn, "func", mcmc_step_fn)  # functools.partial
    module = sys.modules.get(getattr(fn, "__module__", None) or "")
    if module is None or not module.__name__.startswith(__name__.split(".")[0] + "."):
        return None
    infos = [c for name, c in vars(module).items()
             if isinstance(c, type) and name.endswith("Info") and hasattr(c, "_fields")]
    if not infos:
        return None
    return any("acceptance_rate" in c._fields for c in infos)


def build_pretune(mcmc_init_fn: Callable, mcmc_step_fn: Callable, alpha: float, sigma_parameters: dict,
                  n_particles: int, performance_of_chain_measure_factory: Callable = default_measure_factory,
                  positive_parameters=None) -> Callable:
    """blackjax/smc/pretuning.py ``build_pretune``: ``pretune(key, state, logposterior_fn) -> parameter_override``.
    ``state`` is a ``StateWithParameterOverride``; the sampled parameters are the keys of ``sigma_parameters``, each an
    ``(N,)`` or ``(N, K)`` float32 device tensor in ``state.parameter_override``.  The trial is one transition of all
    ``N`` particles from ``state.sampler_state.particles``, keyed like ``update_and_take_last`` with one step (particle
    ``i`` uses ``split(split(key, N)[i], 1)[0]``); ``update_parameter_distribution`` is keyed ``key`` as well, as in
    the reference.  A sampled ``(N, D)`` ``inverse_mass_matrix`` reaches the move tagged as one diagonal per particle
    (``metrics.PerChainDiagTensor``) and comes back tagged.  The move's info must carry ``acceptance_rate``."""
    alpha = _checked_alpha(alpha)
    n_particles = int(n_particles)
    if n_particles < 1:
        raise ValueError("n_particles must be at least 1")
    if not isinstance(sigma_parameters, dict) or not sigma_parameters:
        raise ValueError("sigma_parameters must be a non-empty dict: its keys are the parameters that are sampled")
    positive = tuple(positive_parameters or ())
    unknown = set(positive) - set(sigma_parameters)
    if unknown:
        raise ValueError(f"positive_parameters {sorted(unknown)} are not sampled (not keys of sigma_parameters)")
    if _info_has_acceptance_rate(mcmc_step_fn) is False:
        raise TypeError("pretuning scores a move by its acceptance_rate, which the info of this mcmc_step_fn does not "
                        "carry")
    sigma_cache: dict = {}  # (name, device) -> sigma_parameters[name] on the device, 0-d or (K,): formed once

    def tagged(name, p):
        if name == "inverse_mass_matrix" and p.ndim == 2 and not isinstance(p, metrics.PerChainDiagTensor):
            return metrics.PerChainDiagTensor.tag(p)
        return p

    def pretune(key, state: StateWithParameterOverride, logposterior_fn: Callable) -> dict:
        override = state.parameter_override
        x = base.check_particles(state.sampler_state.particles, "state.sampler_state.particles")
        n = x.shape[0]
        if n != n_particles:
            raise ValueError(f"the pretune was built for {n_particles} particles, the state holds {n}")
        absent = [name for name in sigma_parameters if name not in override]
        if absent:
            raise ValueError(f"the parameter override has no entry for the sampled parameters {absent}")
        sampled = {name: _checked_sample(override[name], name, n) for name in sigma_parameters}
        sigmas = {}
        for name, p in sampled.items():
            hit = sigma_cache.get((name, p.device))
            if hit is None:
                t, stride = _sigma_arg(sigma_parameters[name], 1 if p.ndim == 1 else p.shape[1], p.device, name)
                hit = sigma_cache[(name, p.device)] = t if stride else t.reshape(())
            sigmas[name] = hit
        step_parameters = dict(override)
        step_parameters.update({name: tagged(name, p) for name, p in sampled.items()})
        one_step, _ = base.update_and_take_last(mcmc_init_fn, logposterior_fn, mcmc_step_fn, 1, n)
        moved, info = one_step(key, x, step_parameters)
        if not hasattr(info, "acceptance_rate"):
            raise TypeError(f"pretuning needs the move's acceptance_rate, {type(info).__name__} has none")
        measure_fn = performance_of_chain_measure_factory(StateWithParameterOverride(state.sampler_state,
                                                                                     step_parameters))
        new, _ = update_parameter_distribution(key, sampled, x, moved, measure_fn, alpha, sigmas,
                                               info.acceptance_rate, positive)
        out = dict(override)  # shared entries: the same objects
        out.update({name: tagged(name, p) for name, p in new.items()})
        return out

    return pretune


def build_kernel(smc_algorithm, logprior_fn: Callable, loglikelihood_fn: Callable, mcmc_step_fn: Callable,
                 mcmc_init_fn: Callable, resampling_fn: Callable, pretune_fn: Callable, num_mcmc_steps: int = 10,
                 update_strategy: Callable = base.update_and_take_last, **extra_parameters) -> Callable:
    """blackjax/smc/pretuning.py ``build_kernel``: ``kernel(rng_key, state, **extra_step_parameters) ->
    (StateWithParameterOverride, SMCInfoWithParameterDistribution)``; ``extra_step_parameters`` is ``lmbda=`` for
    ``tempered_smc`` and empty for ``adaptive_tempered_smc``, ``extra_parameters`` passes ``target_ess`` and
    ``root_solver`` to the latter.  ``pretune_fn(rng_key, state, logposterior_fn) -> parameter_override`` is
    ``build_pretune``'s result or any callable of that shape."""
    build, adaptive = _inner_build_kernel(smc_algorithm, "pretuning")
    allowed = {"target_ess", "root_solver"} if adaptive else set()
    unknown = set(extra_parameters) - allowed
    if unknown:
        raise TypeError(f"unexpected extra parameters {sorted(unknown)}: the inner algorithm takes {sorted(allowed)}")
    if adaptive and "target_ess" not in extra_parameters:
        raise TypeError("adaptive_tempered_smc needs target_ess=")
    if not callable(pretune_fn):
        raise TypeError("pretune_fn must be callable: pretune_fn(rng_key, state, logposterior_fn) -> parameters")
    inner = build(logprior_fn, loglikelihood_fn, mcmc_step_fn, mcmc_init_fn, resampling_fn,
                  update_strategy=update_strategy, **extra_parameters)
    logdensity = inner.tempered_logdensity

    def kernel(rng_key, state: StateWithParameterOverride, **extra_step_parameters):
        if not adaptive and "lmbda" not in extra_step_parameters:
            raise TypeError("a step of tempered_smc needs lmbda=")
        keys = split(rng_key, 2)
        step_key, pretune_key = keys[0], keys[1]
        inner_state = state.sampler_state
        logdensity.set_temperature(base.device_scalar(inner_state.lmbda, inner_state.particles.device))
        new_override = pretune_fn(pretune_key, state, logdensity)
        if adaptive:
            new_state, info = inner(step_key, inner_state, num_mcmc_steps, new_override, **extra_step_parameters)
        else:
            lmbda = extra_step_parameters.pop("lmbda")
            new_state, info = inner(step_key, inner_state, num_mcmc_steps, lmbda, new_override,
                                    **extra_step_parameters)
        return (StateWithParameterOverride(new_state, new_override),
                SMCInfoWithParameterDistribution(info, new_override))

    kernel.tempered_logdensity = logdensity
    return kernel


def as_top_level_api(smc_algorithm, logprior_fn: Callable, loglikelihood_fn: Callable, mcmc_step_fn: Callable,
                     mcmc_init_fn: Callable, resampling_fn: Callable, initial_parameter_value, pretune_fn: Callable,
                     num_mcmc_steps: int = 10, update_strategy: Callable = base.update_and_take_last,
                     **extra_parameters) -> SamplingAlgorithm:
    """blackjax/smc/pretuning.py ``as_top_level_api``: ``init(position)``, ``step(rng_key, state,
    **extra_step_parameters)``.  ``initial_parameter_value``: the override of the first step -- the sampled entries
    ``(N,)`` / ``(N, K)`` device tensors, one row per particle, every other entry shared."""
    kernel = build_kernel(smc_algorithm, logprior_fn, loglikelihood_fn, mcmc_step_fn, mcmc_init_fn, resampling_fn,
                          pretune_fn, num_mcmc_steps, update_strategy, **extra_parameters)

    def init_fn(position, rng_key=None):
        del rng_key
        return init(smc_algorithm.init, position, initial_parameter_value)

    def step_fn(rng_key, state, **extra_step_parameters):
        return kernel(rng_key, state, **extra_step_parameters)

    return SamplingAlgorithm(init_fn, step_fn)
