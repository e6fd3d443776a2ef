"""GPU parity of persistent-sampling SMC (blackjax_amd/smc/persistent_sampling.py, adaptive_persistent_sampling.py,
csrc/bjx_smc_persistent.hip, include/bjx_hip.h "SMC") against the NumPy restatement of its arithmetic,
tests/persistent_smc_restatement.py."""
import numpy as np
import pytest
import torch

import blackjax_amd as bjx
import persistent_smc_restatement as rps
import random_walk_restatement as rrw
import smc_restatement as rsmc
from blackjax_amd import _lib, smc
from blackjax_amd import random_walk as prw
from oracle import prng, targets as otargets

pytestmark = pytest.mark.gpu
f32 = np.float32
ps, aps = smc.persistent_sampling, smc.adaptive_persistent_sampling
T = ps.REDUCTION_TILE  # particles per workgroup of the grid-wide reductions

TOL = 1e-6  # den, log-weights and log_Z to TOL * max(1, |value|); normalised weights to TOL
DELTA_TOL = 1e-4  # of the interval searched, as in test_smc_gpu.py


def t2n(t):
    return t.detach().cpu().numpy()


def dev_t(a, dev):
    return torch.as_tensor(np.asarray(a), device=dev)


def assert_close(got, want, what=""):
    """|got - want| <= TOL * max(1, |want|), NaN and infinities in the same places."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), what
    err = np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))
    assert err.size == 0 or err.max() <= TOL, (what, err.max())


def _case(n, i, scale=8.0, pad=1):
    """Slots 0 .. i live, ``pad`` zero slots after them: log-likelihoods -scale z^2, a schedule that starts at 0 and
    rises to 0.6, log_Z_s = log E exp(lambda_s ll) of that distribution."""
    rng = np.random.default_rng(1000 * n + i)
    slots = i + 1 + pad
    pll = np.zeros((slots, n), f32)
    pll[: i + 1] = (-scale * rng.standard_normal((i + 1, n)) ** 2).astype(f32)
    sched = np.zeros(slots, f32)
    sched[: i + 1] = (0.6 * (np.arange(i + 1) / max(i, 1)) ** 2).astype(f32)
    plz = np.zeros(slots, f32)
    plz[: i + 1] = (-0.5 * np.log1p(2.0 * scale * sched[: i + 1].astype(np.float64))).astype(f32)
    return pll, plz, sched


def _check_weights(dev, pll, plz, sched, i, include_current=False):
    """The denominator against the restatement; then the weights kernel against the restatement AT THE DEVICE'S
    denominator (its input: at |ll| = 1e4 one fp32 ulp of den is 1e-3 in a log-weight), normalised log-weights,
    weights and log_Z; then the public functions under both normalisations."""
    n = pll.shape[1]
    n_terms = i + (1 if include_current else 0)
    P = n_terms * n
    g = [dev_t(a, dev) for a in (pll, plz, sched)]
    ll = pll.reshape(-1)[:P]
    den_g = t2n(ps._denominator(*g, n_terms))
    den_r = rps.denominator(ll, sched[:n_terms], plz[:n_terms])
    assert den_g.shape == (P,)
    assert_close(den_g, den_r, "den")
    lw_g, w_g, lz_g = ps._weigh(*g, i, n_terms, True, True)
    lw_r, w_r, lz_r, _ = rps.weigh(sched[i], ll, den_g)
    assert lz_g.shape == () and lw_g.shape == w_g.shape == (P,)
    assert_close(t2n(lz_g), lz_r, "log_Z")
    assert_close(t2n(lw_g), lw_r, "log-weights")
    w = t2n(w_g)
    if np.isnan(w_r).any():  # no particle counts
        assert np.isnan(w).all() and np.isnan(w_r).all() and float(lz_g) == -np.inf
        return
    assert np.array_equal(w == 0, w_r == 0) and np.all(np.isfinite(w))
    assert np.abs(w.astype(np.float64) - w_r).max() <= TOL and abs(w.astype(np.float64).sum() - 1) <= 1e-5
    # the public functions: padded to (T+1, N), -inf / 0 beyond the live rows
    for one in (False, True):
        shift, factor = (0.0, 1.0) if one else (np.log(np.float64(P)), float(P))
        log_w, log_z = ps.compute_log_persistent_weights(*g, i, include_current=include_current, normalize_to_one=one)
        wts, log_z2 = ps.compute_persistent_weights(*g, i, include_current=include_current, normalize_to_one=one)
        assert log_w.shape == wts.shape == pll.shape and torch.equal(log_z, lz_g) and torch.equal(log_z2, lz_g)
        assert_close(t2n(log_w).reshape(-1)[:P], lw_r.astype(np.float64) + shift, "public log-weights")
        np.testing.assert_allclose(t2n(wts).reshape(-1)[:P], w_r.astype(np.float64) * factor, rtol=2e-6,
                                   atol=TOL * factor)
        assert np.all(t2n(log_w).reshape(-1)[P:] == -np.inf) and np.all(t2n(wts).reshape(-1)[P:] == 0)


# one particle; below / above a wavefront multiple; a ragged second tile (i = 2, N = 1000); more than one tile
@pytest.mark.parametrize("n", [1, 65, 1000, 1025])
@pytest.mark.parametrize("i", [1, 2, 7, 33])
def test_weights_match_restatement(dev, n, i):
    _check_weights(dev, *_case(n, i), i)


# P = i * N at the reduction tile less one, at it, one more and twice it plus three
@pytest.mark.parametrize("n,i", [(T - 1, 1), (T, 1), (T + 1, 1), (2 * T + 3, 1), ((T - 1) // 3, 3), (T // 2, 2),
                                 ((T + 1) // 5, 5), ((2 * T + 3) // 7, 7)])
def test_weights_at_the_reduction_tile(dev, n, i):
    assert i * n in (T - 1, T, T + 1, 2 * T + 3)
    _check_weights(dev, *_case(n, i), i)


@pytest.mark.parametrize("n,i", [(65, 2), (1000, 7), (1025, 33)])
def test_weights_with_large_loglikelihoods(dev, n, i):
    """|ll| of order 1e4: exp underflows unless the maximum is subtracted, in the denominator and in the sums."""
    pll, plz, sched = _case(n, i, scale=1e4)
    assert np.abs(pll).max() > 1e4
    _check_weights(dev, pll, plz, sched, i)


@pytest.mark.parametrize("n,i", [(65, 2), (1000, 7)])
def test_weights_with_non_finite_loglikelihoods(dev, n, i):
    """-inf and NaN log-likelihoods: weight exactly 0 (log-weight -inf), never a NaN elsewhere."""
    pll, plz, sched = _case(n, i)
    flat = pll.reshape(-1)
    bad = [3, 17, n + 5, i * n - 1]
    flat[[3, n + 5]] = -np.inf
    flat[[17, i * n - 1]] = np.nan
    _check_weights(dev, pll, plz, sched, i)
    g = [dev_t(a, dev) for a in (pll, plz, sched)]
    w = t2n(ps.compute_persistent_weights(*g, i, normalize_to_one=True)[0]).reshape(-1)
    assert np.all(w[bad] == 0) and np.all(np.isfinite(w)) and abs(w.astype(np.float64).sum() - 1) <= 1e-5


def test_no_particle_of_positive_weight(dev):
    """Every log-likelihood -inf: the weights are NaN and log_Z is -inf, as ``bjx_smc_reweight`` has it."""
    pll, plz, sched = _case(65, 2)
    pll[:2] = -np.inf
    _check_weights(dev, pll, plz, sched, 2)
    g = [dev_t(a, dev) for a in (pll, plz, sched)]
    wts, log_z = ps.compute_persistent_weights(*g, 2, normalize_to_one=True)
    assert float(log_z) == -np.inf and bool(torch.isnan(wts.reshape(-1)[:130]).all())


@pytest.mark.parametrize("n,i", [(65, 1), (1000, 7), (1025, 2)])
def test_weights_including_the_current_iteration(dev, n, i):
    """include_current=True: slots s <= i, i + 1 mixture terms, the temperature of slot i."""
    _check_weights(dev, *_case(n, i), i, include_current=True)


def test_iteration_zero_including_current_is_uniform(dev):
    pll, plz, sched = _case(65, 0)
    _check_weights(dev, pll, plz, sched, 0, include_current=True)
    st = ps.PersistentSMCState(dev_t(np.zeros((2, 65, 3), f32), dev), *[dev_t(a, dev) for a in (pll, plz, sched)], 0)
    w = t2n(st.persistent_weights)
    assert np.abs(w[0] - 1.0).max() <= TOL and np.all(w[0] == w[0, 0]) and np.all(w[1] == 0)


# ----------------------------------------------------------------------------- the solve
def _solve(dev, pll, plz, sched, t, target_ess):
    """-> (delta, lam_new) of the device, (delta, lam_new) of the restatement, the restatement's (ll, den)."""
    n = pll.shape[1]
    P = (t + 1) * n
    g = [dev_t(a, dev) for a in (pll, plz, sched)]
    den = ps._denominator(*g, t + 1)
    delta = torch.empty((), dtype=torch.float32, device=dev)
    lam_new = torch.empty((), dtype=torch.float32, device=dev)
    _lib.call("bjx_smc_persistent_ess_solve", _lib.current_stream(), P, g[0].data_ptr(), den.data_ptr(),
              n * float(target_ess), g[2].data_ptr() + 4 * t, ps._workspace(P, dev).data_ptr(), delta.data_ptr(),
              lam_new.data_ptr())
    st = ps.PersistentSMCState(torch.zeros((pll.shape[0], n, 1), device=dev), *g, t)
    assert torch.equal(aps.calculate_lambda(st, target_ess), lam_new)  # the public function: bit for bit the same
    ll = pll.reshape(-1)[:P]
    den_np = t2n(den)
    d_r, lam_r = rps.solve_lambda(ll, den_np, f32(n * float(target_ess)), sched[t])
    return f32(delta.item()), f32(lam_new.item()), d_r, lam_r, ll, den_np


# t = 0: N particles at temperature 0; t = 2 with a target above N (the persistent set holds more effective
# particles than one iteration has); t = 6: 7 N particles, several tiles.  Every case bisects (from the restatement)
@pytest.mark.parametrize("n", [65, 1000, 1025])
@pytest.mark.parametrize("t,target_ess", [(0, 0.5), (2, 1.3), (6, 3.0)])
def test_solve_matches_restatement(dev, n, t, target_ess):
    pll, plz, sched = _case(n, t)
    delta, lam, d_r, lam_r, ll, den = _solve(dev, pll, plz, sched, t, target_ess)
    width = 1.0 - float(sched[t])
    print("n", n, "t", t, "delta", delta, d_r, "lam", lam, lam_r)
    assert 0 < d_r < f32(width)  # the case bisects
    assert abs(float(delta) - float(d_r)) <= DELTA_TOL * width and abs(float(lam) - float(lam_r)) <= DELTA_TOL * width
    assert lam == f32(sched[t] + delta)
    ess = rps.ess_at(lam, ll, den) / n
    print("achieved ESS / N", ess, "target", target_ess)
    assert target_ess <= ess <= target_ess * 1.01


@pytest.mark.parametrize("n,t,target_ess", [(65, 6, 1.5), (1025, 6, 1.5), (1000, 2, 0.5)])
def test_solve_takes_the_whole_interval_and_lands_on_one(dev, n, t, target_ess):
    pll, plz, sched = _case(n, t)
    delta, lam, d_r, lam_r, _, _ = _solve(dev, pll, plz, sched, t, target_ess)
    assert lam_r == f32(1.0) and lam.view(np.uint32) == f32(1.0).view(np.uint32)
    assert delta == d_r == f32(f32(1.0) - sched[t])


@pytest.mark.parametrize("n,t,target_ess", [(65, 0, 2.0), (1025, 0, 2.0), (1000, 2, 3.0)])
def test_solve_of_an_unreachable_target_does_not_move(dev, n, t, target_ess):
    """No temperature reaches the target: delta == 0 and lam_new == lam_old, bit for bit."""
    pll, plz, sched = _case(n, t)
    delta, lam, d_r, lam_r, _, _ = _solve(dev, pll, plz, sched, t, target_ess)
    assert d_r == 0 and delta.view(np.uint32) == 0
    assert lam.view(np.uint32) == sched[t].view(np.uint32) == lam_r.view(np.uint32)


# ----------------------------------------------------------------------------- full steps
N_STEP = 257


def _step_case(d):
    """The Gaussians of test_smc_gpu._step_case."""
    ivp = np.linspace(0.5, 2.0, d).astype(f32)
    ivl = (np.linspace(1.0, 3.0, d) * (3.5 / np.sqrt(d))).astype(f32)
    x0 = (prng.normal(prng.key(3), (N_STEP, d)) / np.sqrt(ivp)).astype(f32)
    return ivp, ivl, x0


def _inner(name, d):
    if name == "mala":
        tau = f32(0.4 * d ** (-1.0 / 3.0))
        return bjx.mala.build_kernel(), bjx.mala.init, {"step_size": float(tau)}, rsmc.mala_move(tau)
    sigma = 0.5 / np.sqrt(d)  # value-only: additive_step_random_walk with a normal step (normal_random_walk)
    step = rrw.normal(sigma)
    move = rsmc.Move(rrw.init, lambda keys, st, fn: rrw.additive_step_kernel(None, st, fn, step,
                                                                             chain_keys_override=keys))
    return (bjx.additive_step_random_walk.build_kernel(), bjx.additive_step_random_walk.init,
            {"random_step": prw.normal(sigma)}, move)


def _resync(st_g):
    return rps.PersistentSMCState(*[t2n(a).copy() for a in st_g[:4]], st_g.iteration)


def _assert_step(st_g, info_g, st_r, info_r, snapshot):
    i = st_r.iteration
    assert st_g.iteration == i and isinstance(st_g.iteration, int)
    assert info_g.ancestors.dtype == torch.int32 and np.array_equal(t2n(info_g.ancestors), info_r.ancestors)
    assert np.array_equal(t2n(info_g.update_info.is_accepted), info_r.update_info.is_accepted)
    np.testing.assert_allclose(t2n(st_g.particles), st_r.particles, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(t2n(st_g.log_likelihoods), st_r.persistent_log_likelihoods[i], rtol=1e-6, atol=1e-6)
    assert_close(t2n(st_g.log_Z), st_r.log_Z, "log_Z")
    assert f32(st_g.tempering_param.item()) == st_r.tempering_param
    # the step wrote slot i only: every other slot is bit-identical, the padding is zero
    for now, before in zip(st_g[:4], snapshot):
        keep = [s for s in range(now.shape[0]) if s != i]
        assert torch.equal(now[keep].view(torch.int32), before[keep].view(torch.int32))
        assert not bool(now[i + 1:].any())


@pytest.mark.parametrize("d", [3, 64])
@pytest.mark.parametrize("inner", ["mala", "rw"])
@pytest.mark.parametrize("resampling", ["systematic", "stratified"])
def test_persistent_steps_match_restatement(dev, d, inner, resampling):
    """A fixed schedule, then the adaptive sampler from the same start, every step checked from the GPU's own
    previous state: ancestors and accept bits exact, slot contents within 1e-6."""
    ivp, ivl, x0 = _step_case(d)
    prior_r, lik_r = otargets.diag_gaussian(ivp), otargets.diag_gaussian(ivl)
    prior_g, lik_g = bjx.targets.DiagGaussian(dev_t(ivp, dev)), bjx.targets.DiagGaussian(dev_t(ivl, dev))
    step_fn, init_fn, params, move = _inner(inner, d)
    res_g, res_r = getattr(smc.resampling, resampling), getattr(rsmc, resampling)
    n_mcmc = 2
    old_slots = n_acc = n_prop = 0

    fixed = bjx.persistent_sampling_smc(prior_g, lik_g, 5, step_fn, init_fn, params, res_g, num_mcmc_steps=n_mcmc)
    st_g = fixed.init(dev_t(x0, dev))
    st_r = rps.init(x0, lik_r, 5)
    assert st_g.iteration == 0 and st_g.n_particles == N_STEP and st_g.persistent_particles.shape == (6, N_STEP, d)
    np.testing.assert_allclose(t2n(st_g.persistent_log_likelihoods), st_r.persistent_log_likelihoods, rtol=1e-6,
                               atol=1e-6)
    assert np.array_equal(t2n(st_g.persistent_particles), st_r.persistent_particles)
    assert not bool(st_g.persistent_log_Z.any()) and not bool(st_g.tempering_schedule.any())
    for k, lam in zip(prng.split(prng.key(11), 4), (0.05, 0.2, 0.5, 1.0)):
        st_prev, snapshot = _resync(st_g), [a.clone() for a in st_g[:4]]
        st_g, info_g = fixed.step(k, st_g, lam)
        st_r, info_r = rps.step(k, st_prev, f32(lam), prior_r, lik_r, move, n_mcmc, res_r)
        _assert_step(st_g, info_g, st_r, info_r, snapshot)
        assert int(info_r.ancestors.max()) < st_g.iteration * N_STEP
        old_slots += int((info_r.ancestors < (st_g.iteration - 1) * N_STEP).sum())
        n_acc += int(info_r.update_info.is_accepted.sum())
        n_prop += N_STEP
    assert old_slots > 0  # ancestors were drawn from slots older than the last one
    assert 0 < n_acc < n_prop
    with pytest.raises(ValueError):
        fixed.step(prng.key(1), fixed.step(prng.key(2), st_g, 1.0)[0], 1.0)  # a step beyond n_schedule

    adaptive = bjx.adaptive_persistent_sampling_smc(prior_g, lik_g, 6, step_fn, init_fn, params, res_g, 0.9,
                                                    num_mcmc_steps=n_mcmc)
    st_g = adaptive.init(dev_t(x0, dev))
    lams = []
    for k in prng.split(prng.key(12), 6):
        st_prev, snapshot = _resync(st_g), [a.clone() for a in st_g[:4]]
        st_g, info_g = adaptive.step(k, st_g)
        lam_g = f32(st_g.tempering_param.item())
        _, lam_r = rps.calculate_lambda(st_prev, 0.9)
        assert abs(float(lam_g) - float(lam_r)) <= DELTA_TOL * (1.0 - float(st_prev.tempering_param))
        # the rest of the step at the temperature the device chose
        st_r, info_r = rps.step(k, st_prev, lam_g, prior_r, lik_r, move, n_mcmc, res_r)
        _assert_step(st_g, info_g, st_r, info_r, snapshot)
        lams.append(float(lam_g))
        if lam_g == 1:
            break
    print("adaptive temperatures:", lams)
    assert all(b > a for a, b in zip([0.0] + lams, lams)) and lams[-1] <= 1.0


def test_slots_are_written_in_place_and_earlier_states_stay_valid(dev):
    d = 3
    ivp, ivl, x0 = _step_case(d)
    alg = bjx.persistent_sampling_smc(bjx.targets.DiagGaussian(dev_t(ivp, dev)),
                                      bjx.targets.DiagGaussian(dev_t(ivl, dev)), 4, bjx.mala.build_kernel(),
                                      bjx.mala.init, {"step_size": 0.2}, smc.resampling.systematic, num_mcmc_steps=1)
    st0 = alg.init(dev_t(x0, dev))
    st1, _ = alg.step(prng.key(1), st0, 0.3)
    seen = (st1.particles.clone(), st1.log_Z.clone(), st1.tempering_param.clone(), st1.persistent_weights.clone())
    st2, info2 = alg.step(prng.key(2), st1, 0.7)
    # the same buffers, and the earlier states still report their own iteration
    assert st2.persistent_particles.data_ptr() == st0.persistent_particles.data_ptr() and st2.iteration == 2
    assert info2.ancestors.shape == (N_STEP,) and int(info2.ancestors.max()) < 2 * N_STEP
    assert torch.equal(st1.particles, seen[0]) and torch.equal(st1.log_Z, seen[1])
    assert torch.equal(st1.tempering_param, seen[2]) and torch.equal(st1.persistent_weights, seen[3])
    assert np.array_equal(t2n(st0.particles), x0) and float(st0.log_Z) == 0.0 and float(st0.tempering_param) == 0.0
    assert st2.particles.shape == (N_STEP, d) and st2.log_likelihoods.shape == (N_STEP,) and st2.log_Z.shape == ()
    w = st2.persistent_weights
    assert w.shape == (5, N_STEP) and not bool(w[3:].any()) and abs(float(w[:3].mean()) - 1.0) <= 1e-5
    # stepping again from st1 rewrites slot 2 alone
    st2b, _ = alg.step(prng.key(2), st1, 0.7)
    assert torch.equal(st2b.particles, st2.particles) and torch.equal(st2b.log_Z, st2.log_Z)
    trimmed = ps.remove_padding(st2)
    assert trimmed.iteration == 2 and trimmed.persistent_particles.shape == (3, N_STEP, d)
    assert trimmed.persistent_log_likelihoods.shape == (3, N_STEP) and trimmed.persistent_log_Z.shape == (3,)
    assert trimmed.tempering_schedule.shape == (3,) and torch.equal(trimmed.particles, st2.particles)
    assert torch.equal(trimmed.persistent_weights, st2.persistent_weights[:3])
    # compute_log_Z of unnormalised log-weights: log_Z again (the log-weights handed over are rounded to fp32 twice,
    # 1e-6 each at their magnitude of ten or so)
    log_w, log_z = ps.compute_log_persistent_weights(*st2[1:4], 2, include_current=False)
    np.testing.assert_allclose(t2n(ps.compute_log_Z(log_w + log_z, 2)), t2n(st2.log_Z), rtol=1e-5, atol=1e-5)
    # resample_from_persistent: rows of the flat view
    wts, _ = ps.compute_persistent_weights(*trimmed[1:4], 2, include_current=True, normalize_to_one=True)
    x, anc = ps.resample_from_persistent(prng.key(5), trimmed.persistent_particles, wts, smc.resampling.systematic)
    assert torch.equal(x, trimmed.persistent_particles.reshape(-1, d)[anc.long()])
    st3, _ = alg.step(prng.key(3), st2, 0.9)
    st4, _ = alg.step(prng.key(4), st3, 1.0)
    with pytest.raises(ValueError):
        alg.step(prng.key(5), st4, 1.0)  # a step beyond n_schedule


# ----------------------------------------------------------------------------- tracing, end to end, validation
def _conj_torch():
    def logprior(q):
        return -0.5 * (q * q).sum(-1) - 0.5 * rsmc.CONJ_D * float(np.log(2 * np.pi))

    def loglik(q):
        r = q - rsmc.CONJ_Y
        return (-0.5 / rsmc.CONJ_S2) * (r * r).sum(-1) - 0.5 * rsmc.CONJ_D * float(np.log(2 * np.pi * rsmc.CONJ_S2))

    return logprior, loglik


def _counted(fn):
    calls = [0]

    def wrapped(q):
        calls[0] += 1
        return fn(q)

    return wrapped, calls


def test_adaptive_steps_do_not_retrace(dev):
    """Plain PyTorch prior and likelihood under call counters, in the manner of
    test_smc_gpu.test_adaptive_steps_do_not_retrace.  Six adaptive steps with 3 MALA moves evaluate the prior
    6 x (1 + 3) times and the likelihood 1 + 6 x (1 + 3 + 1) times (init; MALA's init and transitions and the moved
    particles' log-likelihoods): neither Python function is called more often than ``value_and_grad(fn)`` calls it
    when evaluated that many times directly, and the run-time compiler's cache does not grow after the first step."""
    from blackjax_amd import rtc
    from blackjax_amd._util import value_and_grad

    logprior, loglik = _conj_torch()
    x0 = dev_t(prng.normal(prng.key(5), (512, rsmc.CONJ_D)), dev)
    n_steps, n_mcmc = 6, 3
    (prior_c, prior_calls), (lik_c, lik_calls) = _counted(logprior), _counted(loglik)
    alg = bjx.adaptive_persistent_sampling_smc(prior_c, lik_c, n_steps, bjx.mala.build_kernel(), bjx.mala.init,
                                               {"step_size": 0.02}, smc.resampling.systematic, 0.9,
                                               num_mcmc_steps=n_mcmc)
    st = alg.init(x0)
    cache_after_first = None
    for k in prng.split(prng.key(6), n_steps):
        st, _ = alg.step(k, st)
        if cache_after_first is None:
            cache_after_first = len(rtc._CODE_CACHE)
    assert len(rtc._CODE_CACHE) == cache_after_first
    assert st.iteration == n_steps and bool(torch.isfinite(st.persistent_weights).all())

    (prior_d, prior_direct), (lik_d, lik_direct) = _counted(logprior), _counted(loglik)
    vg_p, vg_l = value_and_grad(prior_d), value_and_grad(lik_d)
    for _ in range(n_steps * (1 + n_mcmc)):
        vg_p(x0)
    for _ in range(1 + n_steps * (1 + n_mcmc + 1)):
        vg_l(x0)
    print("python calls: prior", prior_calls[0], "direct", prior_direct[0], "likelihood", lik_calls[0], "direct",
          lik_direct[0])
    assert prior_calls[0] <= prior_direct[0] and lik_calls[0] <= lik_direct[0]


def test_custom_root_solver(dev):
    """A ``root_solver`` other than ``solver.dichotomy`` receives ``fun(delta) -> (P,)`` log-weights on the device, the
    target and ``max_delta = 1 - lambda_t`` as a 0-d tensor; a ``delta`` that reaches ``max_delta`` lands on exactly
    1.0, as in ``adaptive_tempered``."""
    d = 3
    ivp, ivl, x0 = _step_case(d)
    prior_g, lik_g = bjx.targets.DiagGaussian(dev_t(ivp, dev)), bjx.targets.DiagGaussian(dev_t(ivl, dev))
    seen = []

    def third(fun, target_ess, max_delta):
        lw = fun(torch.zeros_like(max_delta))
        seen.append((tuple(lw.shape), lw.is_cuda, target_ess, float(max_delta)))
        return max_delta / 3.0

    args = (bjx.mala.build_kernel(), bjx.mala.init, {"step_size": 0.2}, smc.resampling.systematic, 0.9)
    alg = bjx.adaptive_persistent_sampling_smc(prior_g, lik_g, 3, *args, root_solver=third, num_mcmc_steps=1)
    st = alg.init(dev_t(x0, dev))
    st, _ = alg.step(prng.key(1), st)
    assert f32(st.tempering_param.item()) == f32(f32(1.0) / f32(3.0))
    st, _ = alg.step(prng.key(2), st)
    assert seen[0] == ((N_STEP,), True, 0.9, 1.0) and seen[1][0] == (2 * N_STEP,) and abs(seen[1][3] - 2 / 3) < 1e-6
    whole = bjx.adaptive_persistent_sampling_smc(prior_g, lik_g, 3, *args, root_solver=lambda f, t, m: m,
                                                 num_mcmc_steps=1)
    st, _ = whole.step(prng.key(3), st)
    assert torch.equal(st.tempering_param.cpu(), torch.ones((), dtype=torch.float32)) and st.iteration == 3


def test_conjugate_target_end_to_end(dev):
    """The conjugate case of test_persistent_smc_api.py on the device, N = 4 096, target_ess = 0.9, plain PyTorch
    log-densities, ``while state.tempering_param < 1``: ``log_Z`` within 5 x the standard deviation recorded by the
    CPU test, the posterior mean and variance under ``persistent_weights`` within 5 standard errors at the run's
    ESS, which exceeds N; the temperature ends at 1.0 exactly."""
    logprior, loglik = _conj_torch()
    alg = bjx.adaptive_persistent_sampling_smc(logprior, loglik, 24, bjx.mala.build_kernel(), bjx.mala.init,
                                               smc.extend_params({"step_size": rsmc.CONJ_MALA_STEP}),
                                               smc.resampling.systematic, 0.9, num_mcmc_steps=5)
    state = alg.init(dev_t(prng.normal(prng.key(100), (4096, rsmc.CONJ_D)), dev))
    key = prng.key(300)
    while state.tempering_param < 1:
        key, sub = prng.split(key, 2)
        state, _ = alg.step(sub, state)
    assert torch.equal(state.tempering_param.cpu(), torch.ones((), dtype=torch.float32))
    est = float(state.log_Z)
    k = state.iteration + 1
    w = t2n(state.persistent_weights)[:k].reshape(-1).astype(np.float64)
    assert abs(w.mean() - 1.0) <= 1e-5
    w = w / w.sum()
    x = t2n(state.persistent_particles)[:k].reshape(len(w), -1).astype(np.float64)
    mean = (w[:, None] * x).sum(0)
    var = (w[:, None] * (x - mean) ** 2).sum(0)
    ess = 1.0 / np.sum(w * w)
    mean_se = np.abs(mean - rsmc.CONJ_POST_MEAN) / np.sqrt(rsmc.CONJ_POST_VAR / ess)
    var_se = np.abs(var - rsmc.CONJ_POST_VAR) / (rsmc.CONJ_POST_VAR * np.sqrt(2.0 / ess))
    print("log Z", est, "analytic", rsmc.CONJ_LOGZ, "iterations", state.iteration, "ESS", ess, "mean (s.e.)", mean_se,
          "var (s.e.)", var_se)
    assert abs(est - rsmc.CONJ_LOGZ) <= 5.0 * rps.PS_CONJ_LOGZ_SD
    assert np.all(mean_se <= 5.0) and np.all(var_se <= 5.0) and ess > 4096


def test_validation(dev):
    n, d = 16, 4
    g = bjx.targets.DiagGaussian(torch.ones(d, device=dev))
    args = (bjx.mala.build_kernel(), bjx.mala.init, {"step_size": 0.1}, smc.resampling.systematic)
    alg = bjx.persistent_sampling_smc(g, g, 2, *args, num_mcmc_steps=1)
    with pytest.raises(RuntimeError):
        alg.init(torch.zeros(n, d))  # host tensor: there is no CPU fallback
    with pytest.raises(TypeError):
        alg.init(torch.zeros(n, d, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        alg.init(torch.zeros(d, device=dev))  # not (N, D)
    with pytest.raises(ValueError):
        alg.init(torch.zeros(0, d, device=dev))
    with pytest.raises(ValueError):
        bjx.persistent_sampling_smc(g, g, 0, *args)  # n_schedule < 1
    with pytest.raises(ValueError):
        ps.init(torch.zeros(n, d, device=dev), g, 0)
    with pytest.raises(ValueError):
        bjx.adaptive_persistent_sampling_smc(g, g, 4, *args, 0.0)  # target_ess <= 0
    with pytest.raises(ValueError):
        aps.calculate_lambda(alg.init(torch.zeros(n, d, device=dev)), -1.0)
    with pytest.raises(ValueError):  # (n_schedule + 1) * N > 2**24: resampling positions are fp32
        bjx.persistent_sampling_smc(g, g, (1 << 20), *args).init(torch.zeros(n, d, device=dev))
    st = alg.init(torch.zeros(n, d, device=dev))
    with pytest.raises(ValueError):
        ps.compute_log_persistent_weights(*st[1:4], 0)  # no slot before iteration 0
    with pytest.raises(ValueError):
        ps.compute_log_persistent_weights(*st[1:4], 3)  # beyond the slots
    with pytest.raises(ValueError):
        alg.step(prng.key(1), st._replace(persistent_log_likelihoods=st.persistent_log_likelihoods[:, :-1]), 0.5)
