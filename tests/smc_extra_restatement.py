"""NumPy restatement of multinomial / residual resampling, waste-free SMC, inner-kernel tuning and the particle
moments (TEST INFRASTRUCTURE, in the style of smc_restatement.py, which it extends).

Reference functions followed (cited by name: the reference's source is not held next to this file)
* multinomial, residual, _sorted_uniforms            blackjax/smc/resampling.py
* waste_free_smc, update_waste_free                  blackjax/smc/waste_free.py
* build_kernel                                       blackjax/smc/inner_kernel_tuning.py
* particles_means / stds / covariance_matrix         blackjax/smc/tuning/from_particles.py
* update_scale_from_acceptance_rate                  blackjax/smc/tuning/from_kernel_info.py

House numerics (include/bjx_hip.h "SMC"): integer sums only.  Sorted uniforms: ``u_k = uniform(key, (M + 1,))[k]``,
``e_k = -log1p(-u_k)`` correctly rounded to fp32, ``ef_k = floor(e_k * 2^24)``, ``Z = cumsum(ef)``,
``pos_i = Z_i / max(Z_M, 1)`` in fp64.  Multinomial: ``min(N - 1, #{j : C_j < (int64)(pos_i * 2^62)})``.  Residual:
``prod_j = wf_j * M`` exactly, ``cnt_j = prod_j >> 62``, ``rem_j = (prod_j mod 2^62) >> 24``; position ``i < S`` is
``#{j : Ccnt_j <= i}``, position ``i >= S`` is ``min(N - 1, #{j : Crem_j < (int64)(pos_{perm[i]} * (double) Crem[N-1])})``
with the sorted uniforms of ``split(key, 2)[0]`` and ``perm = permutation(split(key, 2)[1], M)``.
"""
from __future__ import annotations

import numpy as np

import smc_restatement as rsmc
from oracle import prng
from oracle.fp import f32, f64, log1p_cr

TWO24 = float(2 ** 24)
MASK62 = (1 << 62) - 1


# ----------------------------------------------------------------------------- resampling
def sorted_uniforms(rng_key, m: int) -> np.ndarray:
    """(m,) fp64 positions, non-decreasing in [0, 1]."""
    u = prng.uniform(rng_key, (int(m) + 1,))
    e = (-log1p_cr(-u)).astype(f32)
    z = np.cumsum(np.floor(e.astype(f64) * TWO24).astype(np.int64))
    return z[:-1].astype(f64) / f64(max(int(z[-1]), 1))


def multinomial(rng_key, weights, num_samples) -> np.ndarray:
    n = len(weights)
    cum = np.cumsum(rsmc.fixed_weights(weights))
    t = (sorted_uniforms(rng_key, num_samples) * rsmc.TWO62).astype(np.int64)
    return np.minimum(np.searchsorted(cum, t, side="left"), n - 1).astype(np.int32)


def residual_split(weights, num_samples):
    """-> (cnt (N,), rem (N,)) int64, through Python integers: the 86-bit product is exact."""
    m = int(num_samples)
    prod = [int(v) * m for v in rsmc.fixed_weights(weights)]
    cnt = np.asarray([p >> 62 for p in prod], np.int64)
    rem = np.asarray([(p & MASK62) >> 24 for p in prod], np.int64)
    return cnt, rem


def residual(rng_key, weights, num_samples) -> np.ndarray:
    n, m = len(weights), int(num_samples)
    keys = prng.split(rng_key, 2)
    cnt, rem = residual_split(weights, m)
    ccnt, crem = np.cumsum(cnt), np.cumsum(rem)
    s = int(ccnt[-1])
    i = np.arange(m)
    certain = np.searchsorted(ccnt, i, side="right")  # #{j : Ccnt_j <= i}
    perm = prng.permutation(keys[1], m)
    pos = sorted_uniforms(keys[0], m)[perm]
    thr = (pos * f64(crem[-1])).astype(np.int64)
    drawn = np.searchsorted(crem, thr, side="left")
    return np.minimum(np.where(i < s, certain, drawn), n - 1).astype(np.int32)


# ----------------------------------------------------------------------------- waste-free, the steps
def waste_free_update(updating_key, x, fn, move: rsmc.Move, p: int):
    """``p - 1`` transitions of the M rows of ``x``, every state kept: rows [0, M) are ``x``, row
    ``M + i (p - 1) + t`` is chain i after transition t + 1.  -> ((M p, D) particles, tuple of the p - 1 infos)."""
    x = np.asarray(x, f32)
    m, d = x.shape
    out = np.empty((m * p, d), f32)
    out[:m] = x
    st = move.init(x, fn)
    chain_keys = prng.split(updating_key, m)
    infos = []
    for t in range(p - 1):
        st, info = move.step(prng.split(chain_keys, 1, offset=t)[:, 0], st, fn)
        out[m + t::p - 1] = np.asarray(st.position, f32)
        infos.append(info)
    return out, tuple(infos)


def tempered_step(rng_key, state, lmbda, logprior_fn, loglikelihood_fn, move: rsmc.Move, num_mcmc_steps,
                  resampling_fn=rsmc.systematic, waste_free_p=None):
    """smc_restatement.tempered_step with an update strategy: ``waste_free_p=None`` is update_and_take_last,
    otherwise N / p ancestors are drawn and ``waste_free_update`` moves them."""
    if waste_free_p is None:
        return rsmc.tempered_step(rng_key, state, lmbda, logprior_fn, loglikelihood_fn, move, num_mcmc_steps,
                                  resampling_fn)
    x, w, lam_old = state
    n = x.shape[0]
    assert n % waste_free_p == 0 and num_mcmc_steps is None
    keys = prng.split(rng_key, 2)
    updating_key, resampling_key = keys[0], keys[1]
    ancestors = resampling_fn(resampling_key, w, n // waste_free_p)
    fn = rsmc.tempered_logdensity(logprior_fn, loglikelihood_fn, lam_old)
    x, infos = waste_free_update(updating_key, x[ancestors], fn, move, waste_free_p)
    ll, _ = loglikelihood_fn(x)
    weights, increment = rsmc.reweight(ll, lam_old, lmbda)
    return rsmc.TemperedSMCState(x, weights, f32(lmbda)), rsmc.SMCInfo(ancestors, increment, infos)


def adaptive_step(rng_key, state, target_ess, logprior_fn, loglikelihood_fn, move: rsmc.Move, num_mcmc_steps,
                  resampling_fn=rsmc.systematic, waste_free_p=None):
    """The next temperature from ALL incoming particles, then the tempered step."""
    ll, _ = loglikelihood_fn(state.particles)
    _, lam_new = rsmc.next_temperature(ll, target_ess, state.lmbda)
    return tempered_step(rng_key, state, lam_new, logprior_fn, loglikelihood_fn, move, num_mcmc_steps, resampling_fn,
                         waste_free_p)


def inner_kernel_tuning_step(rng_key, state, override, lmbda, logprior_fn, loglikelihood_fn, make_move,
                             parameter_update_fn, num_mcmc_steps, resampling_fn=rsmc.systematic, waste_free_p=None):
    """``parameter_update_key, step_key = split(rng_key, 2)``; the tempered step with the move ``make_move(override)``
    keyed ``step_key``; the new override from ``parameter_update_fn(parameter_update_key, new_state, info)``.
    -> (new_state, new_override, info)."""
    keys = prng.split(rng_key, 2)
    new_state, info = tempered_step(keys[1], state, lmbda, logprior_fn, loglikelihood_fn, make_move(override),
                                    num_mcmc_steps, resampling_fn, waste_free_p)
    return new_state, parameter_update_fn(keys[0], new_state, info), info


# ----------------------------------------------------------------------------- moments, tuning
def particles_means(x) -> np.ndarray:
    return np.asarray(x, f32).astype(f64).mean(axis=0).astype(f32)


def particles_stds(x) -> np.ndarray:
    """ddof 0, fp64 throughout, rounded once."""
    return np.asarray(x, f32).astype(f64).std(axis=0).astype(f32)


def particles_covariance_matrix(x) -> np.ndarray:
    """ddof 1, fp64."""
    x = np.asarray(x, f32).astype(f64)
    c = x - x.mean(axis=0)
    return c.T @ c / (x.shape[0] - 1)


def update_scale_from_acceptance_rate(scales, acceptance_rates, target_acceptance_rate=0.234):
    return np.asarray(scales, f64) * np.exp(np.asarray(acceptance_rates, f64) - target_acceptance_rate)
