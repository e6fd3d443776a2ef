"""GPU parity of tempered / adaptive tempered SMC (blackjax_amd/smc/, csrc/bjx_smc.hip, include/bjx_hip.h "SMC")
against the NumPy restatement of the reference's arithmetic, tests/smc_restatement.py."""
import numpy as np
import pytest
import torch

import blackjax_amd as bjx
import smc_restatement as rsmc
from blackjax_amd import smc
from oracle import prng, targets as otargets

pytestmark = pytest.mark.gpu
f32 = np.float32
T = smc.resampling.SCAN_TILE  # items per workgroup of the prefix scan

RTOL, ATOL = 1e-6, 1e-7  # the package's standing tolerances for fp64-summed scalars rounded to fp32
# delta is compared to 1e-4 of the interval searched: the stopping width of the reference's ``dichotomy`` (its ``eps``
# default, as recalled by the issue that specified this test); the device bisection itself stops at 2^-30 of it
DELTA_TOL = 1e-4


def t2n(t):
    return t.detach().cpu().numpy()


def dev_t(a, dev):
    return torch.as_tensor(np.asarray(a), device=dev)


def _weights(n, kind, seed=0):
    rng = np.random.default_rng(1000 * n + seed)
    if kind == "uniform":
        return np.full(n, f32(1.0 / n), f32)
    if kind == "one":  # one weight equal to 1.0, in the middle
        w = np.zeros(n, f32)
        w[n // 2] = 1.0
        return w
    w = rng.random(n) ** 3
    if n > 1:  # exact zeros, w_0 among them
        w[rng.random(n) < 0.2] = 0.0
        w[0] = 0.0
        w[-1] = max(w[-1], 0.1)
    return (w / w.sum()).astype(f32)


def _check_ancestors(dev, n, m, w):
    w_g = dev_t(w, dev)
    for name in ("systematic", "stratified"):
        key = prng.key(7 * n + m)
        a_g = getattr(smc.resampling, name)(key, w_g, m)
        a_r = getattr(rsmc, name)(key, w, m)
        assert a_g.dtype == torch.int32 and a_g.shape == (m,) and a_g.is_cuda
        a = t2n(a_g)
        assert a.min() >= 0 and a.max() < n and np.all(np.diff(a) >= 0)
        assert np.array_equal(a, a_r), (name, n, m, int((a != a_r).sum()))


# below, at and above one wavefront; one tile less one, exactly one, one more (two tiles), three tiles with a ragged
# last one; and T * T + 5, where the tile sums themselves span more than one tile (a third scan level)
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, T - 1, T, T + 1, 2 * T + 3, T * T + 5])
def test_resampling_matches_restatement(dev, n):
    """Ancestors bit for bit, both schemes, weights with exact zeros (w_0 = 0)."""
    _check_ancestors(dev, n, n, _weights(n, "random"))


@pytest.mark.parametrize("n,m,kind", [(1000, 333, "random"), (333, 1000, "random"), (T + 1, 5, "random"),
                                      (65, 65, "one"), (T + 1, 2 * T, "one"), (65, 65, "uniform"),
                                      (T + 1, T + 1, "uniform"), (1, 9, "uniform")])
def test_resampling_other_sample_counts_and_special_weights(dev, n, m, kind):
    _check_ancestors(dev, n, m, _weights(n, kind))


@pytest.mark.parametrize("d", [1, 3, 64, 259, 1032])
def test_gather_is_exact_and_out_of_place(dev, d):
    n, m = 37, 53
    rng = np.random.default_rng(d)
    x = rng.standard_normal((n, d)).astype(f32)
    anc = rng.integers(0, n, m).astype(np.int32)  # unsorted, repeated
    anc[:4] = [n - 1, 0, n - 1, 5]
    x_g = dev_t(x, dev)
    before = x_g.clone()
    out = smc.base.gather(x_g, dev_t(anc, dev))
    assert out.shape == (m, d) and out.data_ptr() != x_g.data_ptr()
    assert np.array_equal(t2n(out).view(np.int32), x[anc].view(np.int32))
    assert torch.equal(x_g, before)


def _loglik_values(n, scale=8.0):
    """-scale z^2: at scale 8 the ESS of delta * ll falls to half of n at delta = 0.32 .. 0.42 for every n used here
    (from the restatement), inside both intervals searched below (0.75 and 0.5), so the solve bisects."""
    return (-scale * np.random.default_rng(n).standard_normal(n) ** 2).astype(f32)


@pytest.mark.parametrize("n", [1, 65, 1000, T + 1])
def test_reweight_and_solve_match_restatement(dev, n):
    ll = _loglik_values(n)
    ll_g = dev_t(ll, dev)
    lam_old = f32(0.25)
    max_delta = f32(f32(1.0) - lam_old)
    # the solve: delta and the new temperature
    delta_g, lam_g = smc.solver.next_temperature(ll_g, 0.5, dev_t(lam_old, dev))
    delta_r, lam_r = rsmc.next_temperature(ll, 0.5, lam_old)
    delta, lam = f32(delta_g.item()), f32(lam_g.item())
    print("n", n, "delta", delta, delta_r, "lam", lam, lam_r)
    assert abs(float(delta) - float(delta_r)) <= DELTA_TOL * float(max_delta)
    assert abs(float(lam) - float(lam_r)) <= DELTA_TOL * float(max_delta)
    ess = np.exp(rsmc.log_ess64(rsmc.log_weights(delta, ll))) / n
    print("achieved ESS / N", ess)
    assert ess >= 0.5
    if n == 1:  # one particle: the ESS is 1 at every delta, the whole interval is taken
        assert delta == max_delta and lam == f32(1.0)
    else:
        assert ess <= 0.5 * 1.01 and 0 < delta < max_delta and lam == f32(lam_old + delta)
    # the same through dichotomy with an explicit interval, and through ess_solver's signature
    d2 = smc.solver.dichotomy(ll_g, 0.5, float(max_delta))
    assert f32(d2.item()) == delta
    # the reweighting at that temperature
    w_g, inc_g, lam_out = smc.base.reweight(ll_g, dev_t(lam_old, dev), lam_g)
    w_r, inc_r = rsmc.reweight(ll, lam_old, lam)
    assert w_g.shape == (n,) and inc_g.shape == () and lam_out.shape == () and f32(lam_out.item()) == lam
    np.testing.assert_allclose(t2n(w_g), w_r, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(t2n(inc_g), inc_r, rtol=RTOL, atol=ATOL)
    # log_ess / ess of explicit log-weights
    lw = rsmc.log_weights(delta, ll)
    np.testing.assert_allclose(t2n(smc.ess.log_ess(dev_t(lw, dev))), rsmc.log_ess(lw), rtol=RTOL, atol=ATOL)
    # ess = exp of the fp32 log_ess (at most log 2^24 = 16.6, so rounded to 1e-6 absolute) by torch.exp in fp32
    np.testing.assert_allclose(t2n(smc.ess.ess(dev_t(lw, dev))), np.exp(rsmc.log_ess64(lw)), rtol=1e-5)


@pytest.mark.parametrize("n", [65, T + 1])
def test_solve_takes_the_whole_interval_and_lands_on_one(dev, n):
    """f(max_delta) >= 0: delta = 1 - lam_old and the new temperature is 1.0 exactly."""
    ll = _loglik_values(n, scale=1e-3)
    lam_old = f32(0.7)
    delta_g, lam_g = smc.solver.next_temperature(dev_t(ll, dev), 0.5, dev_t(lam_old, dev))
    delta_r, lam_r = rsmc.next_temperature(ll, 0.5, lam_old)
    assert lam_r == f32(1.0) and torch.equal(lam_g.cpu(), torch.ones((), dtype=torch.float32))
    assert f32(delta_g.item()) == delta_r == f32(f32(1.0) - lam_old)


@pytest.mark.parametrize("n", [65, 1000])
def test_non_finite_loglikelihoods(dev, n):
    """delta == 0 gives uniform weights whatever the log-likelihoods are (an -inf among them); otherwise -inf and NaN
    entries are particles of weight 0, in the reweighting and in the solve."""
    ll = _loglik_values(n)
    ll[[3, 17]] = -np.inf
    ll[[5, 40]] = np.nan
    ll_g = dev_t(ll, dev)
    lam = dev_t(f32(0.5), dev)
    w0, inc0, _ = smc.base.reweight(ll_g, lam, lam)
    assert np.array_equal(t2n(w0), np.full(n, f32(1.0 / n), f32)) and abs(float(inc0)) <= ATOL
    delta_g, lam_g = smc.solver.next_temperature(ll_g, 0.5, lam)
    delta_r, _ = rsmc.next_temperature(ll, 0.5, f32(0.5))
    assert abs(float(delta_g) - float(delta_r)) <= DELTA_TOL * 0.5 and 0 < float(delta_g) < 0.5
    ess = np.exp(rsmc.log_ess64(rsmc.log_weights(f32(delta_g.item()), ll))) / n
    assert 0.5 <= ess <= 0.505
    w_g, inc_g, _ = smc.base.reweight(ll_g, lam, lam_g)
    w_r, inc_r = rsmc.reweight(ll, f32(0.5), f32(lam_g.item()))
    w = t2n(w_g)
    assert np.all(w[[3, 17, 5, 40]] == 0) and np.all(np.isfinite(w))
    np.testing.assert_allclose(w, w_r, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(t2n(inc_g), inc_r, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("n", [65, T + 1])
def test_log_ess_drops_non_finite_log_weights(dev, n):
    """``-inf`` and NaN log-weights are particles of weight 0: ``log_ess`` is that of the entries that count."""
    lw = rsmc.log_weights(f32(0.4), _loglik_values(n))
    lw[[3, 17, n - 1]] = -np.inf
    lw[[5, 40]] = np.nan
    expected = rsmc.log_ess(lw)
    print("n", n, "log_ess", expected)
    assert np.isfinite(expected) and expected == rsmc.log_ess(lw[np.isfinite(lw)])
    np.testing.assert_allclose(t2n(smc.ess.log_ess(dev_t(lw, dev))), expected, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("n", [65, T + 1])
def test_reweight_with_no_particle_of_positive_weight(dev, n):
    """Every log-likelihood ``-inf`` and the temperature moves: every weight NaN, the increment exactly ``-inf``."""
    ll = np.full(n, -np.inf, f32)
    w_g, inc_g, lam_out = smc.base.reweight(dev_t(ll, dev), dev_t(f32(0.25), dev), dev_t(f32(0.5), dev))
    w_r, inc_r = rsmc.reweight(ll, f32(0.25), f32(0.5))
    assert np.all(np.isnan(w_r)) and inc_r == -np.inf
    assert w_g.shape == (n,) and np.all(np.isnan(t2n(w_g)))
    assert f32(inc_g.item()) == inc_r and f32(lam_out.item()) == f32(0.5)


# ----------------------------------------------------------------------------- full steps
def _step_case(d):
    """Zero-mean diagonal Gaussians as prior and likelihood (bjx.targets.DiagGaussian / oracle diag_gaussian evaluate
    them alike): the likelihood is scaled so that tempering it in takes a few temperatures at target_ess = 0.5."""
    ivp = np.linspace(0.5, 2.0, d).astype(f32)
    ivl = (np.linspace(1.0, 3.0, d) * (3.5 / np.sqrt(d))).astype(f32)
    x0 = (prng.normal(prng.key(3), (257, d)) / np.sqrt(ivp)).astype(f32)
    return ivp, ivl, x0


def _inner(name, d, dev):
    if name == "mala":
        tau = f32(0.4 * d ** (-1.0 / 3.0))
        return (bjx.mala.build_kernel(), bjx.mala.init, {"step_size": float(tau)}, rsmc.mala_move(tau), 3)
    eps, L = f32(0.6 * d ** (-0.25)), 3
    imm = np.ones(d, f32)
    params = {"step_size": float(eps), "inverse_mass_matrix": dev_t(imm, dev), "num_integration_steps": L}
    return bjx.hmc.build_kernel(), bjx.hmc.init, params, rsmc.hmc_move(eps, imm, L), 2


def _resync(st_g):
    return rsmc.TemperedSMCState(t2n(st_g.particles), t2n(st_g.weights), f32(st_g.lmbda.item()))


def _assert_step(st_g, info_g, st_r, info_r, before, snapshot):
    assert info_g.ancestors.dtype == torch.int32 and np.array_equal(t2n(info_g.ancestors), info_r.ancestors)
    assert np.array_equal(t2n(info_g.update_info.is_accepted), info_r.update_info.is_accepted)
    np.testing.assert_allclose(t2n(st_g.particles), st_r.particles, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(t2n(st_g.weights), st_r.weights, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(t2n(info_g.log_likelihood_increment), info_r.log_likelihood_increment, rtol=RTOL,
                               atol=ATOL)
    assert st_g.lmbda.shape == () and st_g.lmbda.dtype == torch.float32 and st_g.lmbda.is_cuda
    for x, x0 in zip(before, snapshot):  # the incoming state's tensors are untouched
        assert torch.equal(x, x0)


@pytest.mark.parametrize("d", [3, 64])
@pytest.mark.parametrize("inner", ["mala", "hmc"])
@pytest.mark.parametrize("resampling", ["systematic", "stratified"])
def test_tempered_steps_match_restatement(dev, d, inner, resampling):
    """A fixed schedule, then the adaptive sampler from the same start.  Every step is checked from the GPU's own
    previous state (a one-ulp weight difference would legitimately move an ancestor of the NEXT step): ancestors and
    accept bits exact, positions within 1e-6, weights and the increment within the standing tolerances."""
    ivp, ivl, x0 = _step_case(d)
    prior_r, lik_r = otargets.diag_gaussian(ivp), otargets.diag_gaussian(ivl)
    prior_g, lik_g = bjx.targets.DiagGaussian(dev_t(ivp, dev)), bjx.targets.DiagGaussian(dev_t(ivl, dev))
    step_fn, init_fn, params, move, n_mcmc = _inner(inner, d, dev)
    res_g, res_r = getattr(smc.resampling, resampling), getattr(rsmc, resampling)
    duplicated = dropped = False
    n_acc = n_prop = 0

    fixed = bjx.tempered_smc(prior_g, lik_g, step_fn, init_fn, params, res_g, num_mcmc_steps=n_mcmc)
    st_g = fixed.init(dev_t(x0, dev))
    assert float(st_g.lmbda) == 0.0 and np.array_equal(t2n(st_g.weights), rsmc.init(x0).weights)
    for k, lam in zip(prng.split(prng.key(11), 4), (0.05, 0.2, 0.5, 1.0)):
        st_prev, snapshot = _resync(st_g), [x.clone() for x in st_g]
        before = st_g
        st_g, info_g = fixed.step(k, st_g, lam)
        st_r, info_r = rsmc.tempered_step(k, st_prev, f32(lam), prior_r, lik_r, move, n_mcmc, res_r)
        _assert_step(st_g, info_g, st_r, info_r, before, snapshot)
        assert f32(st_g.lmbda.item()) == f32(lam)
        counts = np.bincount(info_r.ancestors, minlength=257)
        duplicated, dropped = duplicated or counts.max() >= 2, dropped or counts.min() == 0
        n_acc += int(info_r.update_info.is_accepted.sum())
        n_prop += 257
    assert duplicated and dropped  # across the run a particle was duplicated and one dropped
    assert 0 < n_acc < n_prop

    adaptive = bjx.adaptive_tempered_smc(prior_g, lik_g, step_fn, init_fn, params, res_g, 0.5, num_mcmc_steps=n_mcmc)
    st_g = adaptive.init(dev_t(x0, dev))
    lams = []
    for k in prng.split(prng.key(12), 4):
        st_prev, snapshot = _resync(st_g), [x.clone() for x in st_g]
        before = st_g
        st_g, info_g = adaptive.step(k, st_g)
        lam_g = f32(st_g.lmbda.item())
        ll_prev, _ = lik_r(st_prev.particles)
        _, lam_r = rsmc.next_temperature(ll_prev, 0.5, st_prev.lmbda)
        assert abs(float(lam_g) - float(lam_r)) <= DELTA_TOL * (1.0 - float(st_prev.lmbda))
        # the rest of the step at the temperature the device chose
        st_r, info_r = rsmc.tempered_step(k, st_prev, lam_g, prior_r, lik_r, move, n_mcmc, res_r)
        _assert_step(st_g, info_g, st_r, info_r, before, snapshot)
        lams.append(float(lam_g))
        if lam_g == 1:
            break
    print("adaptive temperatures:", lams)
    assert all(b > a for a, b in zip([0.0] + lams, lams)) and lams[-1] <= 1.0


def test_generic_base_step(dev):
    """``smc.base.step`` with user update and weight functions: ancestors from the incoming weights, the update's
    output reweighted by the normalised exp of ``weight_fn``."""
    n, d = 65, 3
    x0 = prng.normal(prng.key(1), (n, d))
    w0 = _weights(n, "random")
    state = smc.base.SMCState(dev_t(x0, dev), dev_t(w0, dev), {"shift": 0.5})
    key = prng.key(4)
    new, info = smc.base.step(key, state, lambda k, x, p: (x + p["shift"], "moved"), lambda x: -(x * x).sum(-1),
                              smc.resampling.systematic)
    anc = rsmc.systematic(prng.split(key, 2)[1], w0, n)
    assert np.array_equal(t2n(info.ancestors), anc) and info.update_info == "moved"
    x1 = (x0[anc] + f32(0.5)).astype(f32)
    np.testing.assert_allclose(t2n(new.particles), x1, rtol=1e-6, atol=1e-6)
    w_r, inc_r = rsmc.reweight(t2n(-(new.particles * new.particles).sum(-1)), f32(0.0), f32(1.0))
    np.testing.assert_allclose(t2n(new.weights), w_r, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(t2n(info.log_likelihood_increment), inc_r, rtol=RTOL, atol=ATOL)


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
    """Plain PyTorch prior and likelihood under call counters.  Six adaptive steps with 3 MALA moves evaluate the
    prior 6 x (1 + 3) times (MALA's init and transitions) and the likelihood 6 x (1 + 3 + 2) times (the same, the
    solve's and the reweighting's): neither Python function is called more often than ``value_and_grad(fn)`` calls it
    when evaluated that many times directly (a fresh lambda per temperature would be traced at every step), and the
    run-time compiler's cache does not grow after the first step."""
    from blackjax_amd import rtc
    from blackjax_amd._util import value_and_grad

    logprior, loglik = _conj_torch()
    x0 = dev_t(prng.normal(prng.key(5), (512, rsmc.CONJ_D)), dev)
    n_steps, n_mcmc = 6, 3
    (prior_c, prior_calls), (lik_c, lik_calls) = _counted(logprior), _counted(loglik)
    alg = bjx.adaptive_tempered_smc(prior_c, lik_c, bjx.mala.build_kernel(), bjx.mala.init, {"step_size": 0.02},
                                    smc.resampling.systematic, 0.9, num_mcmc_steps=n_mcmc)
    st = alg.init(x0)
    cache_after_first = None
    for k in prng.split(prng.key(6), n_steps):
        st, _ = alg.step(k, st)
        if cache_after_first is None:
            cache_after_first = len(rtc._CODE_CACHE)
    assert len(rtc._CODE_CACHE) == cache_after_first
    assert bool(torch.isfinite(st.weights).all())

    (prior_d, prior_direct), (lik_d, lik_direct) = _counted(logprior), _counted(loglik)
    vg_p, vg_l = value_and_grad(prior_d), value_and_grad(lik_d)
    for _ in range(n_steps * (1 + n_mcmc)):
        vg_p(x0)
    for _ in range(n_steps * (1 + n_mcmc + 2)):
        vg_l(x0)
    print("python calls: prior", prior_calls[0], "direct", prior_direct[0], "likelihood", lik_calls[0], "direct",
          lik_direct[0])
    assert prior_calls[0] <= prior_direct[0] and lik_calls[0] <= lik_direct[0]


def test_conjugate_target_end_to_end(dev):
    """The conjugate case of test_smc_api.py on the device, N = 4 096, plain PyTorch log-densities, ``while
    state.lmbda < 1``: the log evidence within 5 x the standard deviation recorded by the CPU test, the weighted
    posterior mean and variance within 5 standard errors at the run's ESS, the temperature ends at 1.0 exactly."""
    logprior, loglik = _conj_torch()
    alg = bjx.adaptive_tempered_smc(logprior, loglik, bjx.mala.build_kernel(), bjx.mala.init,
                                    smc.extend_params({"step_size": rsmc.CONJ_MALA_STEP}), smc.resampling.systematic,
                                    0.5, num_mcmc_steps=5)
    state = alg.init(dev_t(prng.normal(prng.key(100), (4096, rsmc.CONJ_D)), dev))
    key, total, steps = prng.key(300), torch.zeros((), device=dev), 0
    while state.lmbda < 1:
        key, sub = prng.split(key, 2)
        state, info = alg.step(sub, state)
        total = total + info.log_likelihood_increment
        steps += 1
        assert steps < 50
    assert torch.equal(state.lmbda.cpu(), torch.ones((), dtype=torch.float32))
    est = float(total)
    mean, var, ess = rsmc.weighted_moments(_resync(state))
    mean_se = np.abs(mean - rsmc.CONJ_POST_MEAN) / np.sqrt(rsmc.CONJ_POST_VAR / ess)
    var_se = np.abs(var - rsmc.CONJ_POST_VAR) / (rsmc.CONJ_POST_VAR * np.sqrt(2.0 / ess))
    print("log Z", est, "analytic", rsmc.CONJ_LOGZ, "temperatures", steps, "mean (s.e.)", mean_se, "var (s.e.)", var_se)
    assert abs(est - rsmc.CONJ_LOGZ) <= 5.0 * rsmc.CONJ_LOGZ_SD
    assert np.all(mean_se <= 5.0) and np.all(var_se <= 5.0)


def test_validation(dev):
    n, d = 16, 4
    w = torch.full((n,), 1.0 / n, device=dev)
    key = prng.key(1)
    with pytest.raises(RuntimeError):
        smc.resampling.systematic(key, torch.full((n,), 1.0 / n), n)  # host tensor: there is no CPU fallback
    with pytest.raises(RuntimeError):
        bjx.tempered_smc.init(torch.zeros(n, d))
    with pytest.raises(RuntimeError):
        smc.base.gather(torch.zeros(n, d, device=dev), torch.zeros(n, dtype=torch.int32))
    with pytest.raises(ValueError):
        smc.resampling.systematic(key, w.reshape(4, 4), n)  # not (N,)
    with pytest.raises(ValueError):
        smc.resampling.stratified(key, 2.0 * w, n)  # not normalised
    negative = w.clone()
    negative[0], negative[1] = -1.0 / n, 3.0 / n  # sums to 1, but is not a weight vector
    with pytest.raises(ValueError):
        smc.resampling.systematic(key, negative, n)
    with pytest.raises(ValueError):
        smc.resampling.systematic(key, w, (1 << 24) + 1)  # positions are fp32
    with pytest.raises(ValueError):
        smc.resampling.systematic(key, torch.zeros(0, device=dev), 4)  # N = 0: nothing to draw from
    with pytest.raises(ValueError):
        bjx.tempered_smc.init(torch.zeros(0, d, device=dev))
    with pytest.raises(ValueError):
        bjx.tempered_smc.init(torch.zeros(d, device=dev))  # not (N, D)
    with pytest.raises(ValueError):
        smc.base.gather(torch.zeros(n, d, device=dev), torch.zeros(n, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        smc.solver.dichotomy(torch.zeros(n, device=dev), 1.5, 1.0)  # target_ess is a fraction
    assert smc.resampling.systematic(key, w, 0).shape == (0,)  # no samples asked for: an empty launch
    alg = bjx.tempered_smc(bjx.targets.DiagGaussian(torch.ones(d, device=dev)),
                           bjx.targets.DiagGaussian(torch.ones(d, device=dev)), bjx.mala.build_kernel(), bjx.mala.init,
                           {"step_size": 0.1}, smc.resampling.systematic, num_mcmc_steps=1)
    st = alg.init(torch.zeros(n, d, device=dev))
    with pytest.raises(ValueError):
        alg.step(key, st._replace(weights=w[:-1].contiguous()), 0.5)  # weights of the wrong length
