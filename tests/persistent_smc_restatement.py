"""NumPy restatement of persistent-sampling SMC (TEST INFRASTRUCTURE, in the style of smc_restatement.py, whose
resampling, moves and conjugate target it reuses).

Reference functions followed (cited by name: the reference's source is not held next to this file)
* PersistentSMCState, PersistentStateInfo, init, compute_log_persistent_weights, compute_log_Z,
  resample_from_persistent, step                     blackjax/smc/persistent_sampling.py
* calculate_lambda, build_kernel                     blackjax/smc/adaptive_persistent_sampling.py

The arithmetic, over the ``P = n_terms * N`` rows of slots ``s < n_terms`` at temperature ``lam``:

    den_j = logsumexp_{s < n_terms}(a_sj - logZ_s) - log(n_terms),   a_sj = fp32(lambda_s * ll_j), 0 when lambda_s == 0
            (fp64, the maximum subtracted, summed in index order, rounded once to fp32)
    lw_j  = (double) fp32(lam * ll_j) - (double) den_j               (a NaN or -inf lw_j: weight 0, in no sum)
    logZ  = logsumexp_j(lw_j) - log(P) ;  W_j = exp(lw_j - logsumexp(lw))   (fp64, each rounded once)

and the house bisection of smc_restatement.solve_delta on f(delta) = log_ess(lw(lambda_t + delta)) - log(N target_ess).
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import smc_restatement as rsmc
from oracle import prng
from oracle.fp import f32, f64

HALVINGS = rsmc.HALVINGS

# standard deviation of log_Z over the 16 seeds of
# test_persistent_smc_api.py::test_restatement_is_a_correct_sampler_on_a_conjugate_target (N = 4096, target_ess = 0.9,
# systematic resampling, 5 MALA steps of size 0.1), recorded from that test's own print-out; the device test uses 5 x
# this
PS_CONJ_LOGZ_SD = 0.037


class PersistentSMCState(NamedTuple):
    persistent_particles: np.ndarray  # (T+1, N, D)
    persistent_log_likelihoods: np.ndarray  # (T+1, N)
    persistent_log_Z: np.ndarray  # (T+1,)
    tempering_schedule: np.ndarray  # (T+1,)
    iteration: int

    @property
    def particles(self):
        return self.persistent_particles[self.iteration]

    @property
    def log_Z(self):
        return self.persistent_log_Z[self.iteration]

    @property
    def tempering_param(self):
        return self.tempering_schedule[self.iteration]


class PersistentStateInfo(NamedTuple):
    ancestors: np.ndarray  # (N,) int32 in [0, i * N)
    update_info: object


def init(particles, loglikelihood_fn, n_schedule: int) -> PersistentSMCState:
    x = np.asarray(particles, f32)
    n, d = x.shape
    pp = np.zeros((n_schedule + 1, n, d), f32)
    pll = np.zeros((n_schedule + 1, n), f32)
    pp[0] = x
    pll[0] = loglikelihood_fn(x)[0]
    return PersistentSMCState(pp, pll, np.zeros(n_schedule + 1, f32), np.zeros(n_schedule + 1, f32), 0)


def denominator(loglikelihood, schedule, log_Z) -> np.ndarray:
    """den (P,) f32 of the flat log-likelihoods against the ``n_terms = len(schedule)`` mixture terms."""
    ll = np.asarray(loglikelihood, f32).reshape(-1)
    n_terms = len(schedule)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        terms = [rsmc.log_weights(schedule[s], ll).astype(f64) - f64(f32(log_Z[s])) for s in range(n_terms)]
        m = np.full(ll.shape, -np.inf, f64)
        for t in terms:
            m = np.fmax(m, t)
        total = np.zeros(ll.shape, f64)
        for t in terms:  # index order
            total = total + np.exp(t - m)
        return (m + np.log(total) - np.log(f64(n_terms))).astype(f32)


def log_weights64(lam, loglikelihood, den) -> np.ndarray:
    """lw (P,) f64: the difference of two fp32 values, exact."""
    with np.errstate(invalid="ignore", over="ignore"):
        return rsmc.log_weights(lam, loglikelihood).astype(f64) - np.asarray(den, f32).astype(f64)


def _counts(lw) -> np.ndarray:
    return ~np.isnan(lw) & (lw != -np.inf)


def weigh(lam, loglikelihood, den):
    """-> (normalised log-weights (P,) f32, weights (P,) f32, log_Z f32, lse f64)."""
    lw = log_weights64(lam, np.asarray(loglikelihood, f32).reshape(-1), den)
    ok = _counts(lw)
    P = lw.shape[0]
    if not ok.any():
        return np.full(P, np.nan, f32), np.full(P, np.nan, f32), f32(-np.inf), -np.inf
    m = lw[ok].max()
    with np.errstate(invalid="ignore", over="ignore"):
        lse = m + np.log(np.sum(np.exp(lw[ok] - m)))
        log_w = np.full(P, -np.inf, f64)
        log_w[ok] = lw[ok] - lse
        w = np.zeros(P, f64)
        w[ok] = np.exp(lw[ok] - lse)
    return log_w.astype(f32), w.astype(f32), f32(lse - np.log(f64(P))), lse


def persistent_log_weights(pll, plz, schedule, iteration, include_current=False, normalize_to_one=False):
    """compute_log_persistent_weights -> (log_weights (T+1, N) f32, -inf beyond the live slots ; log_Z f32 ;
    weights (T+1, N) f32, 0 beyond the live slots, under the same normalisation)."""
    n_terms = iteration + (1 if include_current else 0)
    n = pll.shape[1]
    P = n_terms * n
    ll = pll.reshape(-1)[:P]
    den = denominator(ll, schedule[:n_terms], plz[:n_terms])
    log_w, w, log_z, _ = weigh(schedule[iteration], ll, den)
    log_w, w = log_w.astype(f64), w.astype(f64)
    if not normalize_to_one:
        log_w, w = log_w + np.log(f64(P)), w * P
    out_lw = np.full(pll.shape, -np.inf, f32)
    out_w = np.zeros(pll.shape, f32)
    out_lw.reshape(-1)[:P] = log_w
    out_w.reshape(-1)[:P] = w
    return out_lw, log_z, out_w


def log_ess64(lw64) -> float:
    """2 log S1 - log S2 of fp64 log-weights, S_k = sum exp(k (lw - max)) over the particles that count."""
    ok = _counts(lw64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        e = np.exp(lw64[ok] - (lw64[ok].max() if ok.any() else 0.0))
        return float(2.0 * np.log(np.sum(e)) - np.log(np.sum(e * e)))


def ess_at(lam, loglikelihood, den) -> float:
    return float(np.exp(log_ess64(log_weights64(lam, np.asarray(loglikelihood, f32).reshape(-1), den))))


def solve_lambda(loglikelihood, den, target, lam_old):
    """-> (delta f32, lam_new f32); ``target`` is the ABSOLUTE effective sample size (N * target_ess), taken in fp32.
    f(1 - lam_old) >= 0: the whole interval and lam_new = 1 exactly; else 30 halvings in fp32, left end returned."""
    ll = np.asarray(loglikelihood, f32).reshape(-1)
    lam_old = f32(lam_old)
    log_target = float(np.log(f64(f32(target))))

    def f(d):
        return log_ess64(log_weights64(f32(lam_old + f32(d)), ll, den)) - log_target

    max_delta = f32(f32(1.0) - lam_old)
    if f(max_delta) >= 0:
        return max_delta, f32(1.0)
    lo, hi = f32(0.0), max_delta
    for _ in range(HALVINGS):
        mid = f32(f32(0.5) * f32(lo + hi))
        if f(mid) >= 0:
            lo = mid
        else:
            hi = mid
    return lo, f32(lam_old + lo)


def calculate_lambda(state: PersistentSMCState, target_ess):
    """-> (delta, lam_new) over the (t + 1) * N rows the next step weighs."""
    t = state.iteration
    n = state.persistent_log_likelihoods.shape[1]
    ll = state.persistent_log_likelihoods.reshape(-1)[: (t + 1) * n]
    den = denominator(ll, state.tempering_schedule[: t + 1], state.persistent_log_Z[: t + 1])
    return solve_lambda(ll, den, f32(n * float(target_ess)), state.tempering_schedule[t])


def step(rng_key, state: PersistentSMCState, lmbda, logprior_fn, loglikelihood_fn, move: rsmc.Move,
         num_mcmc_steps: int, resampling_fn=rsmc.systematic):
    """persistent_sampling.py::step: weigh the rows of slots s < i at the new temperature, draw N ancestors in
    [0, i N), move at the NEW temperature, fill slot i (of copies: the incoming state is left alone)."""
    pp, pll, plz, sched = (a.copy() for a in state[:4])
    slots, n, d = pp.shape
    i = state.iteration + 1
    if i >= slots:
        raise ValueError("all iterations are taken")
    lam = f32(lmbda)
    sched[i] = lam
    keys = prng.split(rng_key, 2)
    updating_key, resampling_key = keys[0], keys[1]
    P = i * n
    ll = pll.reshape(-1)[:P]
    _, w, log_z, _ = weigh(lam, ll, denominator(ll, sched[:i], plz[:i]))
    ancestors = resampling_fn(resampling_key, w, n)
    x = pp.reshape(-1, d)[:P][ancestors]
    fn = rsmc.tempered_logdensity(logprior_fn, loglikelihood_fn, lam)
    st = move.init(x, fn)
    info = None
    chain_keys = prng.split(updating_key, n)
    for t in range(num_mcmc_steps):
        st, info = move.step(prng.split(chain_keys, 1, offset=t)[:, 0], st, fn)
    x = np.asarray(st.position, f32)
    pp[i], pll[i], plz[i] = x, loglikelihood_fn(x)[0], log_z
    return PersistentSMCState(pp, pll, plz, sched, i), PersistentStateInfo(ancestors, info)


def adaptive_step(rng_key, state: PersistentSMCState, target_ess, logprior_fn, loglikelihood_fn, move: rsmc.Move,
                  num_mcmc_steps: int, resampling_fn=rsmc.systematic):
    """adaptive_persistent_sampling.py::build_kernel: the next temperature, then the step."""
    _, lam_new = calculate_lambda(state, target_ess)
    return step(rng_key, state, lam_new, logprior_fn, loglikelihood_fn, move, num_mcmc_steps, resampling_fn)


def persistent_moments(state: PersistentSMCState):
    """-> (mean (D,), variance (D,), ESS) of all (iteration + 1) * N particles under ``persistent_weights``
    (include_current=True), fp64."""
    k = state.iteration + 1
    _, _, w = persistent_log_weights(state.persistent_log_likelihoods, state.persistent_log_Z,
                                     state.tempering_schedule, state.iteration, include_current=True)
    w = w[:k].reshape(-1).astype(f64)
    w = w / w.sum()
    x = state.persistent_particles[:k].reshape(len(w), -1).astype(f64)
    mean = (w[:, None] * x).sum(0)
    var = (w[:, None] * (x - mean) ** 2).sum(0)
    return mean, var, 1.0 / np.sum(w * w)
