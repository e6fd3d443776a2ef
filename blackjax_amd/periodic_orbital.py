"""Batched periodic orbital MCMC on MI355X behind the ``blackjax.orbital_hmc`` API surface.

Mirrors blackjax/mcmc/periodic_orbital.py (Neklyudov & Welling 2022): ``PeriodicOrbitalState``, ``PeriodicOrbitalInfo``,
``init``, ``build_kernel`` (``kernel`` with ``periodic_orbital_proposal``) and ``as_top_level_api``.  The state of a
chain is a whole weighted orbit of ``period`` samples.  A transition selects one slot of it with probability equal to
its weight, draws ONE momentum, and rebuilds every slot ``j`` by ONE application of the bijection to the selected
state with the signed step ``(j - d) * step_size`` (``d`` the selected slot's direction); the new weights are the
softmax of ``logdensity - kinetic_energy`` over the orbit.  There is no accept / reject and no trajectory loop: a
transition of ``N`` chains is one log-density call on ``N * period`` independent rows.

The chain axis is native; chain ``i`` of ``step(rng_key, state)`` follows the reference's single-chain
``step(jax.random.split(rng_key, N)[chain_offset + i], state_i)``.  ``step_size`` may be a per-chain ``(N,)`` tensor;
``inverse_mass_matrix`` is a shared ``(D,)`` diagonal or per-chain ``(N, D)`` diagonals (``metrics.default_metric``); a
dense matrix is not implemented.  Like every RNG-dependent part of the package, parity with a real JAX run is unpinned
(DESIGN.md section 3); the arithmetic is held against a NumPy restatement (tests/orbital_hmc_restatement.py).

``bijection`` is ``integrators.velocity_verlet`` (the fused path) or a callable with the reference's signature,
``bijection(logdensity_fn, kinetic_energy_fn) -> one_step(state, step_size)``, which is what expresses a truly
periodic flow (for a Gaussian target: the exact rotation with ``step_size = 2 pi / period``).  It is called with batched
torch versions of both functions; ``one_step`` receives an ``IntegratorState`` of ``N * period`` rows (the selected
state repeated) and the ``(N * period,)`` tensor of signed steps, and returns an ``IntegratorState`` of the same shapes.

One deliberate deviation from the reference: its softmax turns a single NaN log-weight into NaN weights for the whole
orbit, after which the chain never recovers.  Here a log-weight that is NaN or ``+inf`` becomes ``-inf`` -- the slot
gets weight exactly 0 -- in the spirit of ``safe_energy_diff``.  The selected slot itself is always part of the new
orbit (signed step 0), so the weights are well defined whenever the incoming state is finite.

The arithmetic runs in libbjxhip (include/bjx_hip.h, "Periodic orbital"); this module sequences
open (one launch) -> user callable on the ``(N * period, D)`` rows -> finish (one launch).
"""
from __future__ import annotations

from typing import Callable, NamedTuple

import torch

from . import _lib, integrators, metrics
from ._util import check_batch, eval_into, eval_logdensity, step_size_args, value_and_grad
from .base import SamplingAlgorithm
from .hmc import IntegratorState
from .random import key_spec

__all__ = ["PeriodicOrbitalState", "PeriodicOrbitalInfo", "init", "build_kernel", "as_top_level_api"]


class PeriodicOrbitalState(NamedTuple):
    """blackjax/mcmc/periodic_orbital.py ``PeriodicOrbitalState``, batched: (N, P, D), (N, P), (N, P) int32, (N, P),
    (N, P, D)."""

    positions: torch.Tensor
    weights: torch.Tensor
    directions: torch.Tensor
    logdensities: torch.Tensor
    logdensities_grad: torch.Tensor


class PeriodicOrbitalInfo(NamedTuple):
    """blackjax/mcmc/periodic_orbital.py ``PeriodicOrbitalInfo``, batched: (N, P, D), (N,), (N,)."""

    momentums: torch.Tensor
    weights_mean: torch.Tensor
    weights_variance: torch.Tensor


def _check_period(period) -> int:
    if isinstance(period, bool) or not isinstance(period, int):
        raise ValueError(f"period must be a positive int, got {period!r}")
    if period < 1:
        raise ValueError(f"period must be at least 1, got {period}")
    return period


def init(position: torch.Tensor, logdensity_fn: Callable, period: int) -> PeriodicOrbitalState:
    """blackjax/mcmc/periodic_orbital.py ``init``: every slot holds the initial position with weight ``1 / period``.
    The reference evaluates the log-density on ``period`` identical copies; here it is evaluated once per chain."""
    position = check_batch(position, "position")
    if position.ndim != 2:
        raise ValueError(f"position must be (n_chains, dim), got {tuple(position.shape)}")
    P = _check_period(period)
    N, D = position.shape
    logp, grad = eval_logdensity(value_and_grad(logdensity_fn), position)
    dev = position.device
    return PeriodicOrbitalState(
        position[:, None, :].expand(N, P, D).contiguous(),
        torch.full((N, P), 1.0 / P, dtype=torch.float32, device=dev),
        torch.arange(P, dtype=torch.int32, device=dev).expand(N, P).contiguous(),
        logp[:, None].expand(N, P).contiguous(),
        grad[:, None, :].expand(N, P, D).contiguous())


_DENSE = ("orbital_hmc: a dense inverse_mass_matrix is not implemented; pass a shared (D,) diagonal or per-chain "
          "(N, D) diagonals (metrics.PerChainDiag / PerChainDiagTensor)")


def _prologue(state: PeriodicOrbitalState, step_size, inverse_mass_matrix, period):
    """The validated inputs of one transition: ``state, N, P, D, metric, eps, eps_pc``."""
    P = _check_period(period)
    q = check_batch(state.positions, "state.positions")
    w = check_batch(state.weights, "state.weights")
    logp = check_batch(state.logdensities, "state.logdensities")
    g = check_batch(state.logdensities_grad, "state.logdensities_grad")
    if q.ndim != 3:
        raise ValueError(f"state.positions must be (n_chains, period, dim), got {tuple(q.shape)}")
    N, Ps, D = q.shape
    if Ps != P:
        raise ValueError(f"period is {P} but the state holds orbits of {Ps} slots")
    d = state.directions
    if not isinstance(d, torch.Tensor) or d.dtype != torch.int32 or d.device != q.device:
        raise TypeError("state.directions must be an int32 tensor on the device of state.positions")
    for name, t, shape in (("weights", w, (N, P)), ("directions", d, (N, P)), ("logdensities", logp, (N, P)),
                           ("logdensities_grad", g, (N, P, D))):
        if tuple(t.shape) != shape:
            raise ValueError(f"state.{name} must be {shape}, got {tuple(t.shape)}")
    metric = metrics.default_metric(inverse_mass_matrix, N, D, q.device)
    if metric.kind != "diag":
        raise NotImplementedError(_DENSE)
    eps, eps_pc = step_size_args(step_size, N, q.device)
    return PeriodicOrbitalState(q, w, d.contiguous(), logp, g), N, P, D, metric, eps, eps_pc


def _open(rng_key, state, N, P, D, metric, eps, eps_pc, chain_offset, drift: bool):
    """``bjx_orbital_open``: -> ``(q, p, step, choice, logp_rep, g_rep)`` with ``N * P`` rows (the last two only for
    ``drift=False``).  ``choice`` (N,) int32 is device-only workspace that the tests read."""
    k0, k1, fold = key_spec(rng_key)
    dev = state.positions.device
    q = torch.empty((N * P, D), dtype=torch.float32, device=dev)
    p = torch.empty_like(q)
    step = torch.empty(N * P, dtype=torch.float32, device=dev)
    choice = torch.empty(N, dtype=torch.int32, device=dev)
    logp_rep = g_rep = None
    if not drift:
        logp_rep, g_rep = torch.empty_like(step), torch.empty_like(q)
    _lib.call("bjx_orbital_open", _lib.current_stream(), k0, k1, int(chain_offset), fold, N, P, D, int(drift), eps,
              _lib.ptr(eps_pc), metric.imm.data_ptr(), metric.imm_stride, state.weights.data_ptr(),
              state.directions.data_ptr(), state.positions.data_ptr(), state.logdensities.data_ptr(),
              state.logdensities_grad.data_ptr(), q.data_ptr(), p.data_ptr(), step.data_ptr(), choice.data_ptr(),
              _lib.ptr(logp_rep), _lib.ptr(g_rep))
    return q, p, step, choice, logp_rep, g_rep


def _finish(N, P, D, metric, step, p_in, logp, g, kick: bool):
    """``bjx_orbital_finish``: -> ``(momentums (N, P, D), weights (N, P), directions (N, P), mean (N,), variance (N,))``."""
    dev = p_in.device
    mom = torch.empty((N, P, D), dtype=torch.float32, device=dev)
    w = torch.empty((N, P), dtype=torch.float32, device=dev)
    dirs = torch.empty((N, P), dtype=torch.int32, device=dev)
    mean = torch.empty(N, dtype=torch.float32, device=dev)
    var = torch.empty(N, dtype=torch.float32, device=dev)
    _lib.call("bjx_orbital_finish", _lib.current_stream(), N, P, D, int(kick), metric.imm.data_ptr(), metric.imm_stride,
              step.data_ptr(), p_in.data_ptr(), logp.data_ptr(), _lib.ptr(g), mom.data_ptr(), w.data_ptr(),
              dirs.data_ptr(), mean.data_ptr(), var.data_ptr())
    return mom, w, dirs, mean, var


def _batched_fns(vg, metric, P):
    """The two functions a user bijection is built from, over ``N * P`` rows: the log-density (its ``value_and_grad``
    attribute returns the pair) and the kinetic energy of ``gaussian_euclidean``, ``0.5 * dot(imm * p, p)``."""

    def logdensity(q):
        return eval_logdensity(vg, q)[0]

    logdensity.value_and_grad = lambda q: eval_logdensity(vg, q)

    def kinetic_energy(p):
        imm = metric.imm if metric.imm_stride == 0 else metric.imm.repeat_interleave(P, dim=0)
        return 0.5 * (imm * p * p).sum(-1)

    return logdensity, kinetic_energy


def _transition(rng_key, state, logdensity_fn, step_size, inverse_mass_matrix, period, bijection, chain_offset):
    """One transition; returns ``(new_state, info, choice, step)`` (the last two for the tests)."""
    state, N, P, D, metric, eps, eps_pc = _prologue(state, step_size, inverse_mass_matrix, period)
    vg = value_and_grad(logdensity_fn)
    fused = bijection is integrators.velocity_verlet
    q, p, step, choice, logp_rep, g_rep = _open(rng_key, state, N, P, D, metric, eps, eps_pc, chain_offset, fused)
    if fused:
        logp, g = eval_into(vg, q, torch.empty_like(step), torch.empty_like(q))
        p_in = p
    else:
        one_step = bijection(*_batched_fns(vg, metric, P))
        out = one_step(IntegratorState(q, p, logp_rep, g_rep), step)
        if not (isinstance(out, tuple) and len(out) == 4):
            raise TypeError("the bijection's one_step must return an IntegratorState")
        q, p_in, logp, g = (check_batch(t, f"one_step(...).{n}") for t, n in zip(out, IntegratorState._fields))
        for name, t, shape in (("position", q, (N * P, D)), ("momentum", p_in, (N * P, D)),
                               ("logdensity", logp, (N * P,)), ("logdensity_grad", g, (N * P, D))):
            if tuple(t.shape) != shape:
                raise ValueError(f"one_step(...).{name} must be {shape}, got {tuple(t.shape)}")
    mom, w, dirs, mean, var = _finish(N, P, D, metric, step, p_in, logp, g if fused else None, fused)
    new_state = PeriodicOrbitalState(q.view(N, P, D), w, dirs, logp.view(N, P), g.view(N, P, D))
    return new_state, PeriodicOrbitalInfo(mom, mean, var), choice, step


def _check_bijection(bijection):
    if isinstance(bijection, integrators.Integrator):
        integrators.check_supported(bijection)
    elif not callable(bijection):
        raise TypeError("bijection must be integrators.velocity_verlet or a callable "
                        "bijection(logdensity_fn, kinetic_energy_fn) -> one_step(state, step_size)")


def build_kernel(bijection=integrators.velocity_verlet):
    """blackjax/mcmc/periodic_orbital.py ``build_kernel``."""
    _check_bijection(bijection)

    def kernel(rng_key, state: PeriodicOrbitalState, logdensity_fn: Callable, step_size, inverse_mass_matrix,
               period: int, *, chain_offset: int = 0):
        return _transition(rng_key, state, logdensity_fn, step_size, inverse_mass_matrix, period, bijection,
                           chain_offset)[:2]

    return kernel


def as_top_level_api(logdensity_fn: Callable, step_size, inverse_mass_matrix, period: int, *,
                     bijection=integrators.velocity_verlet, chain_offset: int = 0) -> SamplingAlgorithm:
    """blackjax/mcmc/periodic_orbital.py ``as_top_level_api``: ``init(position)``, ``step(rng_key, state)``."""
    kernel = build_kernel(bijection)

    def init_fn(position, rng_key=None):
        del rng_key
        return init(position, logdensity_fn, period)

    def step_fn(rng_key, state):
        return kernel(rng_key, state, logdensity_fn, step_size, inverse_mass_matrix, period,
                      chain_offset=chain_offset)

    return SamplingAlgorithm(init_fn, step_fn)
