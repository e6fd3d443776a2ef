"""NumPy restatement of the periodic orbital transition (TEST INFRASTRUCTURE, in the style of tests/mala_restatement.py).

Batched with a leading chain axis; chain ``i`` of ``kernel(rng_key, state, ...)`` follows the reference's single-chain
``blackjax.orbital_hmc.build_kernel()(jax.random.split(rng_key, N)[chain_offset + i], state_i, ...)``.

Reference functions followed (cited by name: the reference's source is not held next to this file)
* PeriodicOrbitalState / PeriodicOrbitalInfo / init   blackjax/mcmc/periodic_orbital.py
* kernel (build_kernel)                               blackjax/mcmc/periodic_orbital.py
* periodic_orbital_proposal (generate)                blackjax/mcmc/periodic_orbital.py
* gaussian_euclidean (sample_momentum, kinetic_energy) blackjax/mcmc/metrics.py
* velocity_verlet                                     blackjax/mcmc/integrators.py
* choice (with p=), _uniform                          jax/_src/random.py
* softmax                                             jax/_src/nn/functions.py

What one transition of a chain does: ``key_momentum, key_select = split(chain key, 2)``; the slot ``i`` is drawn with
``choice(key_select, P, p=weights)``; one momentum is drawn for the selected position; every slot ``j`` of the new
orbit is ONE application of the bijection to the selected state with the signed step
``float32(j - directions[i]) * step_size`` (not ``|j - d|`` applications of ``step_size``); the new weights are
``softmax(logdensity - kinetic_energy)`` over the orbit and the new directions ``arange(P)``.

House numerics: every ``x + s * y`` one fused multiply-add, reductions in fp64 rounded once,
scalar transcendentals in fp64 rounded once.  ``choice``: each prefix of the cumulative sum is accumulated in fp64 and
rounded once; ``1 - u`` and the product with the total are fp32 operations.  ``softmax``: ``exp`` in fp64 rounded once,
the sum in fp64 rounded once, the division in fp32.  Mean and (population) variance of the weights: fp64, rounded once.
Parity of the random streams with a real JAX run is unpinned, as for the rest of the RNG-dependent surface.

One deliberate deviation from the reference: a log-weight that is NaN or ``+inf`` becomes ``-inf`` (weight exactly 0).
The reference's softmax would turn it into NaN weights for the whole orbit, from which the chain never recovers.  The
selected slot itself (signed step 0) is always in the new orbit, so the sum is positive whenever the state is finite.
"""
from __future__ import annotations

from typing import Callable, NamedTuple

import numpy as np

from oracle import prng
from oracle.fp import exp_cr, f32, f64  # (fma32 and dot64 are the arithmetic of the oracle.hmc functions below)
from oracle.hmc import IntegratorState, default_metric, kinetic_energy, sample_momentum, velocity_verlet


class PeriodicOrbitalState(NamedTuple):
    positions: np.ndarray  # (N, P, D)
    weights: np.ndarray  # (N, P)
    directions: np.ndarray  # (N, P) int32
    logdensities: np.ndarray  # (N, P)
    logdensities_grad: np.ndarray  # (N, P, D)


class PeriodicOrbitalInfo(NamedTuple):
    momentums: np.ndarray  # (N, P, D)
    weights_mean: np.ndarray  # (N,)
    weights_variance: np.ndarray  # (N,)


def init(position, logdensity_fn: Callable, period: int) -> PeriodicOrbitalState:
    """Every slot holds the initial position, weight 1 / P, directions arange(P).  The reference evaluates the
    log-density on P identical copies; one evaluation broadcast gives the same values."""
    position = np.asarray(position, dtype=f32)
    N, D = position.shape
    P = int(period)
    logp, grad = logdensity_fn(position)
    logp, grad = np.asarray(logp, f32), np.asarray(grad, f32)
    return PeriodicOrbitalState(
        np.repeat(position[:, None, :], P, axis=1),
        np.full((N, P), f32(1.0) / f32(P), f32),
        np.tile(np.arange(P, dtype=np.int32), (N, 1)),
        np.repeat(logp[:, None], P, axis=1),
        np.repeat(grad[:, None, :], P, axis=1))


def choice(keys, weights):
    """``jax.random.choice(key, P, p=weights)`` per row: ``r = cum[-1] * (1 - uniform(key, ()))``,
    ``searchsorted(cum, r, side="left")`` = the number of ``cum_j < r``, clipped to P - 1."""
    P = weights.shape[1]
    cum = np.cumsum(weights.astype(f64), axis=1).astype(f32)
    u = prng.uniform(keys, ())
    r = (cum[:, -1] * (f32(1.0) - u).astype(f32)).astype(f32)
    with np.errstate(invalid="ignore"):
        below = (cum < r[:, None]).sum(axis=1)
    return np.minimum(below, P - 1).astype(np.int64)


def _rows_metric(inverse_mass_matrix, N, P):
    """The metric over the N chains and the same metric over the N * P rows of an orbit."""
    imm = np.asarray(inverse_mass_matrix, dtype=f32)
    if imm.ndim == 1:
        m = default_metric(imm)
        return m, m
    if imm.ndim == 2 and imm.shape[0] == N:  # (square N == D reads as per-chain here: dense is not restated)
        return (default_metric(imm, per_chain_diag=True),
                default_metric(np.repeat(imm, P, axis=0), per_chain_diag=True))
    raise NotImplementedError("orbital_hmc restates diagonal metrics only: (D,) or (N, D)")


def softmax_weights(logw):
    """``softmax(logw, axis=1)`` with the deviation of the module docstring; -> (weights, mean, population variance)."""
    logw = np.asarray(logw, f32)
    P = logw.shape[1]
    logw = np.where(np.isnan(logw) | (logw == f32(np.inf)), f32(-np.inf), logw).astype(f32)
    m = logw.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        e = exp_cr((logw - m).astype(f32))
    S = e.astype(f64).sum(axis=1, keepdims=True).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = (e / S).astype(f32)
    w64 = w.astype(f64)
    mean64 = w64.sum(axis=1) / P
    var64 = ((w64 - mean64[:, None]) ** 2).sum(axis=1) / P
    return w, mean64.astype(f32), var64.astype(f32)


def kernel(rng_key, state: PeriodicOrbitalState, logdensity_fn, step_size, inverse_mass_matrix, period: int,
           chain_offset: int = 0, chain_keys_override=None, bijection=None):
    """One transition of every chain -> ``(new_state, info, choice)``: the third value is the (N,) index of the slot
    each chain selected.  ``step_size``: a scalar or (N,).  ``chain_keys_override``: (N, 2) per-chain keys used instead of
    ``split(rng_key, .)[chain_offset : chain_offset + N]`` (the chain-major key layout).  ``bijection``: ``None`` is
    velocity Verlet; otherwise a callable with the reference's signature, ``bijection(logdensity_fn, kinetic_energy_fn)
    -> one_step(state, step_size)``, given batched NumPy functions (``logdensity_fn`` returns ``(logp, grad)`` like the
    oracle's targets) and called on an ``IntegratorState`` of N * P rows with the (N * P,) signed steps."""
    q_all, w, dirs, logp_all, g_all = state
    N, P, D = q_all.shape
    assert P == int(period)
    metric, metric_rows = _rows_metric(inverse_mass_matrix, N, P)
    eps = np.broadcast_to(np.asarray(step_size, dtype=f32), (N,)).astype(f32)
    keys = prng.split(rng_key, N, offset=chain_offset) if chain_keys_override is None else chain_keys_override
    kk = prng.split(keys, 2)  # key_momentum, key_select
    i = choice(kk[:, 1], w)
    rows = np.arange(N)
    q, logp, g, d = q_all[rows, i], logp_all[rows, i], g_all[rows, i], dirs[rows, i]
    p = sample_momentum(metric, kk[:, 0], D)

    # direction * step_size, an fp32 product per slot
    signed = ((np.arange(P, dtype=np.int32)[None, :] - d[:, None]).astype(f32) * eps[:, None]).astype(f32).reshape(N * P)
    rep = lambda x: np.repeat(x, P, axis=0)  # noqa: E731  (the selected state, once per slot)
    z = IntegratorState(rep(q), rep(p), rep(logp), rep(g))
    with np.errstate(all="ignore"):
        if bijection is None:
            z = velocity_verlet(z, signed, logdensity_fn, metric_rows)
        else:
            z = bijection(logdensity_fn, lambda mom: kinetic_energy(metric_rows, mom))(z, signed)
            z = IntegratorState(*(np.asarray(x, f32) for x in z))
        logw = (z.logdensity - kinetic_energy(metric_rows, z.momentum)).astype(f32).reshape(N, P)
    weights, mean, var = softmax_weights(logw)
    new_state = PeriodicOrbitalState(z.position.reshape(N, P, D), weights, np.tile(np.arange(P, dtype=np.int32), (N, 1)),
                                     z.logdensity.reshape(N, P), z.logdensity_grad.reshape(N, P, D))
    return new_state, PeriodicOrbitalInfo(z.momentum.reshape(N, P, D), mean, var), i


# ------------------------------------------------------------------------------- the periodic case, shared by the tests
def gaussian_exact_flow(inverse_mass_matrix):
    """A bijection in the reference's signature: the exact Hamiltonian flow of the Gaussian target N(0, diag(imm)) under
    the metric ``imm``, ``q' = q cos t + imm p sin t``, ``p' = p cos t - q sin t / imm``.  It has period 2 pi in ``t``, so
    with ``step_size = 2 pi / period`` the orbit closes and every slot has the same energy.  cos / sin are evaluated in
    fp64 from the fp32 step and rounded once; the rest is fp32, one rounding per operation, in the order written."""
    imm = np.asarray(inverse_mass_matrix, f32)

    def bijection(logdensity_fn, kinetic_energy_fn):
        def one_step(state, step_size):
            q, p = state.position, state.momentum
            t = np.asarray(step_size, f32).astype(f64)[:, None]
            c, s = np.cos(t).astype(f32), np.sin(t).astype(f32)
            q1 = (q * c + (imm * p) * s).astype(f32)
            p1 = (p * c - (q * s) / imm).astype(f32)
            logp, g = logdensity_fn(q1)
            return IntegratorState(q1, p1, np.asarray(logp, f32), np.asarray(g, f32))

        return one_step

    return bijection


def exact_flow_case():
    """The stationarity experiment of the CPU and GPU tests: -> (N, P, sigma, imm, q0, step_size, keys of the 20
    transitions).  N(0, diag(sigma^2)) with sigma = (0.5, 1, 3), imm = sigma^2, every chain started at 3 sigma."""
    N, P = 2048, 8
    sigma = np.array([0.5, 1.0, 3.0], f32)
    imm = (sigma * sigma).astype(f32)
    q0 = np.tile((f32(3.0) * sigma).astype(f32), (N, 1))
    return N, P, sigma, imm, q0, f32(2.0 * np.pi / P), prng.split(prng.key(31), 20)


def weighted_moment_z_scores(positions, weights, sigma):
    """Per chain the weighted first and second moments of its orbit, sum_j w_j q_j and sum_j w_j q_j^2; their averages
    over the chains against 0 and sigma^2 in units of the standard error the across-chain spread gives: -> (2, D)."""
    w = np.asarray(weights, f64)[:, :, None]
    q = np.asarray(positions, f64)
    n = q.shape[0]
    out = []
    for m, target in (((w * q).sum(1), 0.0 * sigma.astype(f64)), ((w * q * q).sum(1), sigma.astype(f64) ** 2)):
        out.append((m.mean(0) - target) / (m.std(0, ddof=1) / np.sqrt(n)))
    return np.stack(out)
