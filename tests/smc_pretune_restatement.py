"""NumPy restatement of pretuned tempered SMC (TEST INFRASTRUCTURE, in the style of smc_extra_restatement.py, which it
extends).

Reference functions followed (cited by name: the reference's source is not held next to this file)
* esjd, update_parameter_distribution, default_measure_factory,
  build_pretune, build_kernel                         blackjax/smc/pretuning.py

House numerics (include/bjx_hip.h "SMC", pretuning).  ESJD: ``d = prev - next`` in fp32, ``s_i = sum_j d_j^2 / imm_j``
in fp64, ``measure_i = (float)(s_i * (double) acc_i)``; NaN, +-inf and negative measures are 0.  Weights:
``t = alpha + measure`` and its sum in fp64, ``w = t / S`` rounded once, uniform when ``S == 0``.  Ancestors:
``smc_extra_restatement.multinomial`` (a deliberate deviation from the reference's ``jax.random.choice``).  Jitter:
``z = normal(noise_key, (N, K))``, the noise of the SOURCE row, ``fma(sigma, z, p)`` or, in log space,
``p * exp(sigma * z)`` with the product and the exponential each rounded to fp32.  The trial transition is keyed like
``update_and_take_last`` with one step, and ``update_parameter_distribution`` with the same key, as in the reference.
"""
from __future__ import annotations

import numpy as np

import mala_restatement as rmala
import smc_extra_restatement as rx
import smc_restatement as rsmc
from oracle import hmc as ohmc
from oracle import prng
from oracle.fp import exp_cr, f32, f64, fma32


# ----------------------------------------------------------------------------- the three kernels
def esjd(prev, nxt, acc, imm=None) -> np.ndarray:
    """(N,) fp32.  ``imm``: None (identity), (D,) shared or (N, D) per particle."""
    prev, nxt = np.asarray(prev, f32), np.asarray(nxt, f32)
    with np.errstate(all="ignore"):
        d = (prev - nxt).astype(f32).astype(f64)
        q = d * d
        if imm is not None:
            q = q / np.asarray(imm, f32).astype(f64)
        m = (q.sum(axis=1) * np.asarray(acc, f32).astype(f64)).astype(f32)
        return np.where(np.isfinite(m) & (m >= 0), m, f32(0.0)).astype(f32)


def esjd_dense64(prev, nxt, acc, imm) -> np.ndarray:
    """(N,) fp64 for a shared dense (D, D) inverse mass matrix, solved in fp64: acc * d^T imm^-1 d."""
    d = (np.asarray(prev, f32) - np.asarray(nxt, f32)).astype(f32).astype(f64)
    y = np.linalg.solve(np.asarray(imm, f32).astype(f64), d.T).T
    return np.asarray(acc, f32).astype(f64) * np.sum(d * y, axis=1)


def pretune_weights(measure, alpha) -> np.ndarray:
    t = f64(f32(alpha)) + np.asarray(measure, f32).astype(f64)
    s = t.sum()
    if s == 0:
        return np.full(t.shape[0], f32(1.0 / t.shape[0]), f32)
    return (t / s).astype(f32)


def jitter_gather(noise_key, p, ancestors, sigma, log_space=False) -> np.ndarray:
    """``p`` (N,) or (N, K), ``ancestors`` (M,) clipped to [0, N), ``sigma`` a scalar or (K,)."""
    p = np.asarray(p, f32)
    n = p.shape[0]
    p2 = p.reshape(n, -1)
    z = prng.normal(noise_key, p2.shape)
    sg = np.broadcast_to(np.asarray(sigma, f32), p2.shape[1:]).astype(f32)[None, :]
    with np.errstate(all="ignore"):
        if log_space:
            out = (p2 * exp_cr((sg * z).astype(f32))).astype(f32)
        else:
            out = fma32(sg, z, p2)
    a = np.clip(np.asarray(ancestors, np.int64), 0, n - 1)
    return out[a].reshape((len(a),) + p.shape[1:])


def update_parameter_distribution(key, params: dict, prev, latest, imm, alpha, sigma_parameters: dict, acc,
                                  positive=()):
    """-> (new parameter samples, measure (N,), weights (N,), ancestors (N,))."""
    keys = prng.split(key, 2)
    noise_key, resampling_key = keys[0], keys[1]
    measure = esjd(prev, latest, acc, imm)
    weights = pretune_weights(measure, alpha)
    ancestors = rx.multinomial(resampling_key, weights, len(weights))
    new = {name: jitter_gather(noise_key, p, ancestors, sigma_parameters[name], name in positive)
           for name, p in params.items()}
    return new, measure, weights, ancestors


def near_boundary(resampling_key, weights, rel=2.0 ** -20) -> np.ndarray:
    """(N,) bool: positions of ``multinomial(resampling_key, weights, N)`` whose threshold lies within ``rel``
    (relative) of a cumulative-weight boundary -- where weights that differ in the last place may move an ancestor."""
    cum = np.cumsum(rsmc.fixed_weights(weights)).astype(f64)
    t = (rx.sorted_uniforms(resampling_key, len(weights)) * rsmc.TWO62).astype(np.int64).astype(f64)
    j = np.clip(np.searchsorted(cum, t, side="left"), 0, len(cum) - 1)
    gap = np.minimum(np.abs(cum[j] - t), np.abs(cum[np.maximum(j - 1, 0)] - t))
    return gap <= rel * np.maximum(t, 1.0)


# ----------------------------------------------------------------------------- moves with per-particle parameters
def mala_move(step_size) -> rsmc.Move:
    """``step_size`` (N,): mala_restatement.kernel broadcasts a scalar and takes a vector as one value per chain."""
    tau = np.asarray(step_size, f32)
    return rsmc.Move(rmala.init, lambda keys, st, fn: rmala.kernel(None, st, fn, tau, chain_keys_override=keys))


def hmc_move(step_size, inverse_mass_matrix, num_integration_steps) -> rsmc.Move:
    """``step_size`` (N,), ``inverse_mass_matrix`` (D,) or one diagonal per particle (N, D)."""
    eps, imm = np.asarray(step_size, f32), np.asarray(inverse_mass_matrix, f32)
    return rsmc.Move(ohmc.init, lambda keys, st, fn: ohmc.kernel(None, st, fn, eps, imm, num_integration_steps,
                                                                 chain_keys_override=keys,
                                                                 per_chain_diag=imm.ndim == 2))


def make_move(kind: str, num_integration_steps: int = 3):
    """-> ``override -> Move`` for "mala" (``step_size``) or "hmc" (``step_size``, ``inverse_mass_matrix``)."""
    if kind == "mala":
        return lambda override: mala_move(override["step_size"])
    return lambda override: hmc_move(override["step_size"], override["inverse_mass_matrix"], num_integration_steps)


# ----------------------------------------------------------------------------- pretune, the step
def pretune(key, particles, override: dict, fn, move_of, alpha, sigma_parameters: dict, positive=()):
    """One trial transition of every particle with its own parameters, then ``update_parameter_distribution``.
    -> (new override, details = (moved particles, acceptance rate, measure, weights, ancestors))."""
    x = np.asarray(particles, f32)
    n = x.shape[0]
    move = move_of(override)
    st = move.init(x, fn)
    chain_keys = prng.split(key, n)
    st, info = move.step(prng.split(chain_keys, 1, offset=0)[:, 0], st, fn)
    moved, acc = np.asarray(st.position, f32), np.asarray(info.acceptance_rate, f32)
    sampled = {name: override[name] for name in sigma_parameters}
    new, measure, weights, ancestors = update_parameter_distribution(
        key, sampled, x, moved, override.get("inverse_mass_matrix"), alpha, sigma_parameters, acc, positive)
    return {**override, **new}, (moved, acc, measure, weights, ancestors)


def pretuned_step(rng_key, state: rsmc.TemperedSMCState, override: dict, lmbda, logprior_fn, loglikelihood_fn, move_of,
                  num_mcmc_steps, alpha, sigma_parameters, positive=(), resampling_fn=rsmc.systematic,
                  target_ess=None):
    """``step_key, pretune_key = split(rng_key, 2)``; the pretune at the state's temperature; the tempered step with
    the new override keyed ``step_key``.  ``lmbda=None`` solves for the next temperature (``target_ess``).
    -> (new_state, new_override, info)."""
    keys = prng.split(rng_key, 2)
    step_key, pretune_key = keys[0], keys[1]
    fn = rsmc.tempered_logdensity(logprior_fn, loglikelihood_fn, state.lmbda)
    new_override, _ = pretune(pretune_key, state.particles, override, fn, move_of, alpha, sigma_parameters, positive)
    if lmbda is None:
        ll, _ = loglikelihood_fn(state.particles)
        _, lmbda = rsmc.next_temperature(ll, target_ess, state.lmbda)
    new_state, info = rsmc.tempered_step(step_key, state, lmbda, logprior_fn, loglikelihood_fn, move_of(new_override),
                                         num_mcmc_steps, resampling_fn)
    return new_state, new_override, info


# ----------------------------------------------------------------------------- the case of the full-step tests
CASE_N, CASE_D, CASE_ALPHA, CASE_L = 64, 3, 0.05, 3
CASE_LMBDA = f32(0.3)  # the temperature of the lone pretune call
CASE_POSITIVE = {"mala": ("step_size",), "hmc": ("step_size", "inverse_mass_matrix")}
# the keys of the pretune call and of the two steps: chosen so that, in the restatement, no threshold of the parameter
# resampling lies within 2^-20 of a cumulative-weight boundary (test_smc_pretune_api.py checks it on the CPU)
CASE_KEYS = {"mala": (21, 22, 23), "hmc": (31, 32, 33)}


def step_case(inner: str):
    """-> (prior inverse variances, likelihood inverse variances, particles (N, D), override, sigma_parameters): the
    zero-mean diagonal Gaussians of test_smc_gpu.py's step case at N = 64, D = 3, with step sizes spread
    log-uniformly over a decade and, for "hmc", one inverse mass diagonal per particle."""
    n, d = CASE_N, CASE_D
    ivp = np.linspace(0.5, 2.0, d).astype(f32)
    ivl = (np.linspace(1.0, 3.0, d) * (3.5 / np.sqrt(d))).astype(f32)
    x0 = (prng.normal(prng.key(3), (n, d)) / np.sqrt(ivp)).astype(f32)
    u = prng.uniform(prng.key(4), (n,)).astype(f64)
    if inner == "mala":
        return ivp, ivl, x0, {"step_size": (0.05 * 10.0 ** u).astype(f32)}, {"step_size": f32(0.1)}
    imm = (0.5 + prng.uniform(prng.key(5), (n, d)).astype(f64)).astype(f32)
    override = {"step_size": (0.08 * 10.0 ** u).astype(f32), "inverse_mass_matrix": imm,
                "num_integration_steps": CASE_L}
    sigma = {"step_size": f32(0.1), "inverse_mass_matrix": np.array([0.05, 0.1, 0.15], f32)}
    return ivp, ivl, x0, override, sigma
