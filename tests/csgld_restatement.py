"""NumPy restatement of contour SGLD (TEST INFRASTRUCTURE, in the style of tests/sgmcmc_restatement.py).

Batched with a leading chain axis; every chain has its own energy histogram.  Chain ``i`` of
``csgld_kernel(rng_key, ...)`` follows the reference's single-chain kernel called with
``jax.random.split(rng_key, N)[chain_offset + i]``.

Reference functions followed (cited by name: the reference's source is not held next to this file)
* ContourSGLDState, init, build_kernel (kernel), as_top_level_api      blackjax/sgmcmc/csgld.py
* overdamped_langevin                                                  blackjax/sgmcmc/diffusions.py

House numerics: every ``x + s * y`` one fused multiply-add, scalars in fp32 in the order written,
log and pow in fp64 rounded once, divisions correctly rounded fp32.  ``csgld_kernel_f64`` is the reference's lines in
plain float64 without any of that, for the self-check of the house version.

An estimator here is any callable over NumPy arrays: ``gradient_estimator(position (N, D), minibatch) -> (N, D)``,
``logdensity_estimator(position (N, D), minibatch) -> (N,)``.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from oracle import prng
from oracle.fp import f32, fma32, log_cr, sqrt32

from sgmcmc_restatement import _chain_keys, _per_chain


class ContourSGLDState(NamedTuple):
    position: np.ndarray  # (N, D) fp32
    energy_pdf: np.ndarray  # (N, M) fp32
    energy_idx: np.ndarray  # (N,) int32


def init(position, num_partitions=512) -> ContourSGLDState:
    """csgld.py init: energy_pdf = arange(M, 0, -1) / sum(arange(M, 0, -1)), energy_idx = M - 1, for every chain."""
    q = np.asarray(position, f32)
    M = int(num_partitions)
    row = (np.arange(M, 0, -1).astype(f32) / f32(M * (M + 1) // 2)).astype(f32)
    return ContourSGLDState(q, np.tile(row, (q.shape[0], 1)), np.full(q.shape[0], M - 1, np.int32))


def multiplier(energy_pdf, energy_idx, zeta, temperature, energy_gap):
    """1 + zeta T (log pdf[i] - log pdf[i - 1]) / energy_gap per chain, (N, 1); the index clamped into [1, M - 1] as
    the engine clamps it on read."""
    pdf = np.asarray(energy_pdf, f32)
    N, M = pdf.shape
    T = _per_chain(temperature, N)[:, 0]
    i = np.clip(np.asarray(energy_idx).astype(np.int64), 1, M - 1)
    rows = np.arange(N)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = (log_cr(pdf[rows, i]) - log_cr(pdf[rows, i - 1])).astype(f32)
        m = f32(1.0) + (((f32(zeta) * T).astype(f32) * d).astype(f32) / f32(energy_gap)).astype(f32)
    return m.astype(f32)[:, None]


def langevin_step(rng_key, position, logdensity_grad, energy_pdf, energy_idx, step_size_diff, temperature=1.0,
                  zeta=1.0, energy_gap=10.0, chain_offset: int = 0, chain_keys_override=None):
    """diffusions.py overdamped_langevin on multiplier * grad: q + eps (m g) + sqrt(2 T eps) normal(chain key)."""
    q = np.asarray(position, f32)
    N, D = q.shape
    eps, T = _per_chain(step_size_diff, N), _per_chain(temperature, N)
    keys = _chain_keys(rng_key, N, chain_offset, chain_keys_override)
    m = multiplier(energy_pdf, energy_idx, zeta, temperature, energy_gap)
    z = prng.normal(keys, (D,))
    s = sqrt32(((f32(2.0) * T).astype(f32) * eps).astype(f32))
    with np.errstate(invalid="ignore", over="ignore"):
        mg = (m * np.asarray(logdensity_grad, f32)).astype(f32)
        return fma32(s, z, fma32(eps, mg, q))


def energy_index(logdensity, num_partitions, energy_gap=10.0, min_energy=0.0):
    """min(max(floor((-logdensity - min_energy) / energy_gap + 1), 1), M - 1) in fp32; a NaN gives 1 (the reference
    converts NaN to 0 and clamps), -inf energy 1, +inf energy M - 1."""
    ld = np.asarray(logdensity, f32)
    M = int(num_partitions)
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.floor((((-ld - f32(min_energy)).astype(f32) / f32(energy_gap)).astype(f32) + f32(1.0)).astype(f32))
        idx = np.where(~(x >= 1), 1.0, np.where(x >= M - 1, float(M - 1), x))
    return idx.astype(np.int32)


def update_energy_histogram(logdensity, energy_pdf, step_size_stoch, zeta=1.0, energy_gap=10.0, min_energy=0.0):
    """pdf + eps_sa pdf[i]^zeta (e_i - pdf) with pdf[i] of the OLD histogram at the NEW index; -> (pdf, idx)."""
    pdf = np.asarray(energy_pdf, f32)
    N, M = pdf.shape
    idx = energy_index(logdensity, M, energy_gap, min_energy)
    rows = np.arange(N)
    a = pdf[rows, idx]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a_zeta = a if float(zeta) == 1.0 else np.power(a.astype(np.float64), float(zeta)).astype(f32)
        w = (_per_chain(step_size_stoch, N)[:, 0] * a_zeta).astype(f32)
        u = -pdf
        u[rows, idx] = (f32(1.0) - a).astype(f32)
        return fma32(w[:, None], u, pdf), idx


def csgld_kernel(rng_key, state: ContourSGLDState, logdensity_estimator, gradient_estimator, minibatch,
                 step_size_diff, step_size_stoch, zeta=1, temperature=1.0, energy_gap=10, min_energy=0,
                 chain_offset: int = 0, chain_keys_override=None) -> ContourSGLDState:
    """csgld.py kernel: gradient at the old position, Langevin step, log-density at the new position, histogram."""
    q, pdf, idx = state
    g = np.asarray(gradient_estimator(np.asarray(q, f32), minibatch), f32)
    q1 = langevin_step(rng_key, q, g, pdf, idx, step_size_diff, temperature, zeta, energy_gap, chain_offset,
                       chain_keys_override)
    ld = np.asarray(logdensity_estimator(q1, minibatch), f32)
    pdf1, idx1 = update_energy_histogram(ld, pdf, step_size_stoch, zeta, energy_gap, min_energy)
    return ContourSGLDState(q1, pdf1, idx1)


def csgld_kernel_f64(rng_key, state, logdensity_estimator, gradient_estimator, minibatch, step_size_diff,
                     step_size_stoch, zeta=1, temperature=1.0, energy_gap=10, min_energy=0, chain_offset: int = 0,
                     chain_keys_override=None) -> ContourSGLDState:
    """The reference's lines in plain float64 (only the normals are the fp32 ones of the chain key).  The estimators
    see float64 positions; whatever the log-density estimator returns is floored as it is."""
    q, pdf, idx = (np.asarray(x) for x in state)
    q, pdf = q.astype(np.float64), pdf.astype(np.float64)
    N, D = q.shape
    M = pdf.shape[1]
    eps = np.broadcast_to(np.asarray(step_size_diff, np.float64), (N,))[:, None]
    T = np.broadcast_to(np.asarray(temperature, np.float64), (N,))[:, None]
    eps_sa = np.broadcast_to(np.asarray(step_size_stoch, np.float64), (N,))
    keys = _chain_keys(rng_key, N, chain_offset, chain_keys_override)
    rows = np.arange(N)
    multiplier = 1.0 + zeta * T[:, 0] * (np.log(pdf[rows, idx]) - np.log(pdf[rows, idx - 1])) / energy_gap
    g = np.asarray(gradient_estimator(q, minibatch), np.float64)
    z = prng.normal(keys, (D,)).astype(np.float64)
    q1 = q + eps * (multiplier[:, None] * g) + np.sqrt(2.0 * T * eps) * z
    neg_logprob = -np.asarray(logdensity_estimator(q1, minibatch), np.float64)
    idx1 = np.clip(np.floor((neg_logprob - min_energy) / energy_gap + 1.0), 1, M - 1).astype(np.int32)
    update = -pdf
    update[rows, idx1] += 1.0
    pdf1 = pdf + (eps_sa * pdf[rows, idx1] ** zeta)[:, None] * update
    return ContourSGLDState(q1, pdf1, idx1)


# ---- a double well, the multimodal target of the step tests ----------------------------------------------------------
# log p(q) = -(|q|^2 - c)^2 / 8: a shell of radius sqrt(c) around a hill at the origin.  The minibatch IS c, a scalar
# that changes every step, so that a minibatch not handed on shows.

def double_well_logdensity_estimator(position, minibatch):
    """-(|q|^2 - c)^2 / 8 in float64."""
    q = np.asarray(position, np.float64)
    return -((q * q).sum(-1) - float(minibatch)) ** 2 / 8.0


def double_well_gradient_estimator(position, minibatch):
    """Its gradient, -((|q|^2 - c) / 2) q, in float64."""
    q = np.asarray(position, np.float64)
    return -(((q * q).sum(-1) - float(minibatch)) / 2.0)[:, None] * q


def double_well_case(N, D, steps=6):
    """-> q0, step_size_diff, step_size_stoch, temperature, minibatches, energy_gap, min_energy.  Chain i starts at
    radius^2 about 4 (0.5 + i / (N - 1))^2, so the chains' energies (|q|^2 - c)^2 / 8 spread over [0, 3] and, with
    energy_gap = 0.25, over a dozen bins.  D > 64: scalar step sizes and temperature; else per-chain ones."""
    radius = (2.0 / np.sqrt(D)) * (0.5 + np.arange(N) / max(N - 1, 1))
    q0 = (prng.normal(prng.key(1), (N, D)) * radius[:, None].astype(f32)).astype(f32)
    rng = np.random.default_rng(1000 * N + D)
    if D > 64:
        eps_diff, eps_stoch, T = 0.002, 0.1, 0.5
    else:
        eps_diff = (f32(0.002) * rng.uniform(0.6, 1.6, N)).astype(f32)
        eps_stoch = (f32(0.1) * rng.uniform(0.5, 1.5, N)).astype(f32)
        T = (f32(0.5) * rng.uniform(0.4, 1.6, N)).astype(f32)
    minibatches = [np.float32(4.0 + 0.5 * np.sin(1.0 + t)) for t in range(steps)]
    return q0, eps_diff, eps_stoch, T, minibatches, 0.25, 0.0
