"""NumPy restatement of tempered and adaptive tempered SMC (TEST INFRASTRUCTURE, in the style of mala_restatement.py).

Reference functions followed (cited by name: the reference's source is not held next to this file)
* SMCState / SMCInfo / step / update_and_take_last   blackjax/smc/base.py
* systematic, stratified                             blackjax/smc/resampling.py
* log_ess, ess_solver                                blackjax/smc/ess.py
* dichotomy                                          blackjax/smc/solver.py
* TemperedSMCState, init, build_kernel               blackjax/smc/tempered.py
* build_kernel (compute_delta)                       blackjax/smc/adaptive_tempered.py

House numerics of the SMC arithmetic (DESIGN.md section 3 and its SMC kernel note): cumulative weights in 2^-62
fixed point (integer sums: exact, whatever the order), positions ``(i + u) / M`` in fp32, the log-sum-exp of the
reweighting in fp64 rounded once, the tempered log-density ``lp + lam * ll`` as an fp32 product followed by an fp32
sum (not fused), the temperature bisection in fp32 with fp64 sums, 30 halvings, left end returned.  The move is the
restatement of the inner sampler (tests/mala_restatement.py, oracle/hmc.py), particle ``i`` keyed
``split(split(updating_key, N)[i], num_mcmc_steps)[t]``.
"""
from __future__ import annotations

from typing import Callable, NamedTuple

import numpy as np

import mala_restatement as rmala
from oracle import hmc as ohmc
from oracle import prng
from oracle.fp import f32, f64

TWO62 = float(2 ** 62)
HALVINGS = 30


class TemperedSMCState(NamedTuple):
    particles: np.ndarray  # (N, D)
    weights: np.ndarray  # (N,)
    lmbda: np.float32


class SMCInfo(NamedTuple):
    ancestors: np.ndarray  # (N,) int32
    log_likelihood_increment: np.float32
    update_info: object


class Move(NamedTuple):
    """The inner sampler: ``init(position, fn) -> state`` ; ``step(chain_keys (N, 2), state, fn) -> (state, info)``."""

    init: Callable
    step: Callable


def mala_move(step_size) -> Move:
    return Move(rmala.init, lambda keys, st, fn: rmala.kernel(None, st, fn, step_size, chain_keys_override=keys))


def hmc_move(step_size, inverse_mass_matrix, num_integration_steps) -> Move:
    return Move(ohmc.init, lambda keys, st, fn: ohmc.kernel(None, st, fn, step_size, inverse_mass_matrix,
                                                            num_integration_steps, chain_keys_override=keys))


def init(particles) -> TemperedSMCState:
    x = np.asarray(particles, f32)
    n = x.shape[0]
    return TemperedSMCState(x, np.full(n, f32(1.0 / n), f32), f32(0.0))


# ----------------------------------------------------------------------------- resampling
def fixed_weights(weights) -> np.ndarray:
    """wf_j = (int64) floor((double) w_j * 2^62), w_j clamped to [0, 1] (NaN -> 0)."""
    w = np.asarray(weights, f32)
    with np.errstate(invalid="ignore"):
        w = np.where(w > 0, np.minimum(w, f32(1.0)), f32(0.0)).astype(f32)
    return np.floor(w.astype(f64) * TWO62).astype(np.int64)


def _ancestors(u, weights, num_samples) -> np.ndarray:
    n, m = len(weights), int(num_samples)
    cum = np.cumsum(fixed_weights(weights))
    pos = ((np.arange(m).astype(f32) + np.asarray(u, f32)).astype(f32) / f32(m)).astype(f32)
    t = (pos.astype(f64) * TWO62).astype(np.int64)  # exact
    return np.minimum(np.searchsorted(cum, t, side="left"), n - 1).astype(np.int32)


def systematic(rng_key, weights, num_samples) -> np.ndarray:
    return _ancestors(prng.uniform(rng_key, ()), weights, num_samples)


def stratified(rng_key, weights, num_samples) -> np.ndarray:
    return _ancestors(prng.uniform(rng_key, (int(num_samples),)), weights, num_samples)


# ----------------------------------------------------------------------------- weights, ESS, temperature
def log_weights(delta, loglikelihood) -> np.ndarray:
    """delta * ll in fp32; delta == 0 gives 0 whatever ll is (the reference's nan_to_num)."""
    ll = np.asarray(loglikelihood, f32)
    if f32(delta) == 0:
        return np.zeros_like(ll)
    with np.errstate(invalid="ignore", over="ignore"):
        return (f32(delta) * ll).astype(f32)


def _counts(lw) -> np.ndarray:
    """A NaN or -inf log-weight is a particle of weight 0."""
    return ~np.isnan(lw) & (lw != -np.inf)


def reweight(loglikelihood, lam_old, lam_new):
    """-> (weights (N,) f32, log_likelihood_increment f32) for lw = (lam_new - lam_old) * ll."""
    delta = f32(f32(lam_new) - f32(lam_old))
    lw = log_weights(delta, loglikelihood)
    ok = _counts(lw)
    n = lw.shape[0]
    if not ok.any():
        return np.full(n, np.nan, f32), f32(-np.inf)
    m = f64(lw[ok].max())
    lse = m + np.log(np.sum(np.exp(lw[ok].astype(f64) - m)))
    w = np.zeros(n, f64)
    w[ok] = np.exp(lw[ok].astype(f64) - lse)
    return w.astype(f32), f32(lse - np.log(f64(n)))


def log_ess64(lw) -> float:
    """2 logsumexp(lw) - logsumexp(2 lw) = 2 log S1 - log S2, S_k = sum exp(k (lw - max)), fp64 throughout."""
    lw = np.asarray(lw, f32)
    ok = _counts(lw)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.exp(lw[ok].astype(f64) - (f64(lw[ok].max()) if ok.any() else 0.0))
        return float(2.0 * np.log(np.sum(e)) - np.log(np.sum(e * e)))


def log_ess(lw) -> np.float32:
    """log_ess64 rounded once to fp32."""
    return f32(log_ess64(lw))


def _f(d, ll, ll_max, log_target) -> float:
    """log_ess(d * ll) - log(N target) as the solve evaluates it: max(d * ll) = d * max(ll), exp and sums in fp64."""
    lw = log_weights(d, ll)
    m = log_weights(d, np.asarray([ll_max], f32))[0]
    ok = _counts(lw)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        e = np.exp(lw[ok].astype(f64) - f64(m))
        return float(2.0 * np.log(np.sum(e)) - np.log(np.sum(e * e)) - log_target)


def solve_delta(loglikelihood, target_ess, max_delta):
    """-> (delta f32, whole): max_delta if the ESS there meets the target, else 30 halvings of [0, max_delta] in
    fp32, the left end moving to mid whenever f(mid) >= 0; the left end is returned."""
    ll = np.asarray(loglikelihood, f32)
    ok = _counts(ll)
    ll_max = f32(ll[ok].max()) if ok.any() else f32(-np.inf)
    log_target = float(np.log(f64(ll.shape[0]) * f64(f32(target_ess))))
    max_delta = f32(max_delta)
    if _f(max_delta, ll, ll_max, log_target) >= 0:
        return max_delta, True
    lo, hi = f32(0.0), max_delta
    for _ in range(HALVINGS):
        mid = f32(f32(0.5) * f32(lo + hi))
        if _f(mid, ll, ll_max, log_target) >= 0:
            lo = mid
        else:
            hi = mid
    return lo, False


def next_temperature(loglikelihood, target_ess, lmbda):
    """-> (delta, lam_new): lam_new is exactly 1 when the whole of 1 - lmbda is taken."""
    lmbda = f32(lmbda)
    delta, whole = solve_delta(loglikelihood, target_ess, f32(f32(1.0) - lmbda))
    return delta, (f32(1.0) if whole else f32(lmbda + delta))


# ----------------------------------------------------------------------------- the steps
def tempered_logdensity(logprior_fn, loglikelihood_fn, lmbda):
    """q -> (lp + lam * ll, gp + lam * gl): fp32 product, then fp32 sum."""
    lam = f32(lmbda)

    def fn(q):
        lp, gp = logprior_fn(q)
        ll, gl = loglikelihood_fn(q)
        with np.errstate(invalid="ignore", over="ignore"):
            logp = (np.asarray(lp, f32) + (lam * np.asarray(ll, f32)).astype(f32)).astype(f32)
            grad = (np.asarray(gp, f32) + (lam * np.asarray(gl, f32)).astype(f32)).astype(f32)
        return logp, grad

    return fn


def tempered_step(rng_key, state: TemperedSMCState, lmbda, logprior_fn, loglikelihood_fn, move: Move,
                  num_mcmc_steps: int, resampling_fn=systematic):
    """base.py::step as called by tempered.py::build_kernel: resample from the incoming weights, move at the OLD
    temperature, reweight with (lam_new - lam_old) * loglikelihood at the moved particles."""
    x, w, lam_old = state
    n = x.shape[0]
    keys = prng.split(rng_key, 2)
    updating_key, resampling_key = keys[0], keys[1]
    ancestors = resampling_fn(resampling_key, w, n)
    x = x[ancestors]
    fn = tempered_logdensity(logprior_fn, loglikelihood_fn, lam_old)
    st = move.init(x, fn)
    info = None
    chain_keys = prng.split(updating_key, n)
    for t in range(num_mcmc_steps):
        st, info = move.step(prng.split(chain_keys, 1, offset=t)[:, 0], st, fn)
    x = np.asarray(st.position, f32)
    ll, _ = loglikelihood_fn(x)
    weights, increment = reweight(ll, lam_old, lmbda)
    return TemperedSMCState(x, weights, f32(lmbda)), SMCInfo(ancestors, increment, info)


def adaptive_step(rng_key, state: TemperedSMCState, target_ess, logprior_fn, loglikelihood_fn, move: Move,
                  num_mcmc_steps: int, resampling_fn=systematic):
    """adaptive_tempered.py::build_kernel: the next temperature from the incoming particles, then the tempered step."""
    ll, _ = loglikelihood_fn(state.particles)
    _, lam_new = next_temperature(ll, target_ess, state.lmbda)
    return tempered_step(rng_key, state, lam_new, logprior_fn, loglikelihood_fn, move, num_mcmc_steps, resampling_fn)


# ----------------------------------------------------------------------------- the conjugate case of the tests
CONJ_D, CONJ_Y, CONJ_S2 = 4, 1.5, 0.25
CONJ_LOGZ = CONJ_D * (-0.5 * np.log(2 * np.pi * (1.0 + CONJ_S2)) - 0.5 * CONJ_Y ** 2 / (1.0 + CONJ_S2))
CONJ_POST_VAR = 1.0 / (1.0 + 1.0 / CONJ_S2)
CONJ_POST_MEAN = CONJ_POST_VAR * CONJ_Y / CONJ_S2
CONJ_MALA_STEP = 0.1
# standard deviation of sum(log_likelihood_increment) over the 16 seeds of
# test_smc_api.py::test_restatement_is_a_correct_sampler_on_a_conjugate_target (N = 4096, target_ess = 0.5, systematic
# resampling, 5 MALA steps of size 0.1), recorded from that test's own print-out; the device test uses 5 x this
CONJ_LOGZ_SD = 0.039


def conj_logprior(q):
    """N(0, I): normalised, so that the increments sum to the log evidence."""
    q = np.asarray(q, f32)
    lp = -0.5 * np.sum(q.astype(f64) ** 2, axis=-1) - 0.5 * q.shape[-1] * np.log(2 * np.pi)
    return lp.astype(f32), (-q).astype(f32)


def conj_loglikelihood(q):
    """N(y | x, 0.25 I), y = 1.5 in every coordinate, normalised."""
    q = np.asarray(q, f32)
    r = (f32(CONJ_Y) - q).astype(f32)
    ll = -0.5 * np.sum(r.astype(f64) ** 2, axis=-1) / CONJ_S2 - 0.5 * q.shape[-1] * np.log(2 * np.pi * CONJ_S2)
    return ll.astype(f32), (r / f32(CONJ_S2)).astype(f32)


def weighted_moments(state: TemperedSMCState):
    """-> (mean (D,), variance (D,), ESS) of the weighted particles, fp64."""
    w = state.weights.astype(f64)
    w = w / w.sum()
    x = state.particles.astype(f64)
    mean = (w[:, None] * x).sum(0)
    var = (w[:, None] * (x - mean) ** 2).sum(0)
    return mean, var, 1.0 / np.sum(w * w)
