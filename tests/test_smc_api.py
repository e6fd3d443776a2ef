"""``blackjax_amd.tempered_smc`` / ``adaptive_tempered_smc`` / ``blackjax_amd.smc``: API surface, C-ABI argument checks
(no GPU needed) and the NumPy restatement the GPU tests hold the kernels against (tests/smc_restatement.py), pinned on
its own as a sampler."""
import numpy as np

import smc_restatement as rsmc
from oracle import prng

f32 = np.float32


def test_smc_api_surface():
    import blackjax_amd as bjx
    from blackjax_amd import smc

    for name in ("tempered_smc", "adaptive_tempered_smc", "smc"):
        assert name in bjx.__all__
    assert bjx.tempered_smc.init is smc.tempered.init and bjx.tempered_smc.build_kernel is smc.tempered.build_kernel
    assert bjx.adaptive_tempered_smc.init is smc.adaptive_tempered.init is smc.tempered.init
    assert bjx.adaptive_tempered_smc.build_kernel is smc.adaptive_tempered.build_kernel
    assert smc.base.SMCState._fields == ("particles", "weights", "update_parameters")
    assert smc.base.SMCInfo._fields == ("ancestors", "log_likelihood_increment", "update_info")
    assert smc.tempered.TemperedSMCState._fields == ("particles", "weights", "lmbda")
    assert rsmc.TemperedSMCState._fields == smc.tempered.TemperedSMCState._fields
    assert rsmc.SMCInfo._fields == smc.base.SMCInfo._fields
    for f in (smc.resampling.systematic, smc.resampling.stratified, smc.ess.ess, smc.ess.log_ess, smc.ess.ess_solver,
              smc.solver.dichotomy, smc.base.step, smc.base.init, smc.extend_params):
        assert callable(f)
    params = {"step_size": 0.1}
    assert smc.extend_params(params) == params and smc.extend_params(params) is not params

    def logprior(q):
        return -0.5 * (q * q).sum(-1)

    def loglik(q):
        return -2.0 * ((q - 1.5) ** 2).sum(-1)

    fixed = bjx.tempered_smc(logprior, loglik, bjx.mala.build_kernel(), bjx.mala.init, params,
                             smc.resampling.systematic, num_mcmc_steps=3)
    adaptive = bjx.adaptive_tempered_smc(logprior, loglik, bjx.mala.build_kernel(), bjx.mala.init, params,
                                         smc.resampling.stratified, 0.5)
    for alg in (fixed, adaptive):
        assert isinstance(alg, bjx.SamplingAlgorithm) and callable(alg.init) and callable(alg.step)
    # ONE tempered log-density per algorithm object, declared as returning (logp, grad) and not recordable (the two
    # plain functions are not); recordable when both callables are
    k = bjx.adaptive_tempered_smc.build_kernel(logprior, loglik, bjx.mala.build_kernel(), bjx.mala.init,
                                               smc.resampling.systematic, 0.5)
    t = k.tempered_logdensity
    assert isinstance(t, smc.tempered.TemperedLogDensity) and t._bjx_returns_pair and not t._bjx_capturable
    from blackjax_amd._util import value_and_grad

    assert value_and_grad(t) is t
    t2 = smc.tempered.TemperedLogDensity(bjx.capturable(logprior), bjx.capturable(loglik))
    assert t2._bjx_capturable


def test_smc_scan_tile_and_workspace_without_gpu():
    from blackjax_amd import _lib
    from blackjax_amd.smc import resampling

    lib = _lib.load()
    T = lib.bjx_smc_scan_tile()
    assert T == resampling.SCAN_TILE
    assert lib.bjx_smc_resample_workspace_bytes(1) == 8 and lib.bjx_smc_resample_workspace_bytes(T) == 8 * T
    assert lib.bjx_smc_resample_workspace_bytes(T + 1) == 8 * (T + 1 + 2)  # + two tile sums
    assert lib.bjx_smc_resample_workspace_bytes(T * T + 1) == 8 * (T * T + 1 + (T + 1) + 2)  # + a second level
    assert lib.bjx_smc_resample_workspace_bytes(0) == 0 and lib.bjx_smc_resample_workspace_bytes((1 << 24) + 1) == 0


def test_smc_entry_points_reject_bad_arguments_without_gpu():
    from blackjax_amd import _lib

    lib = _lib.load()
    calls = {
        "bjx_smc_resample": lambda n, m: lib.bjx_smc_resample(None, 1, 2, 0, n, m, None, None, None),
        "bjx_smc_gather": lambda n, m: lib.bjx_smc_gather(None, n, m, 8, None, None, None),
        "bjx_smc_temper": lambda n, m: lib.bjx_smc_temper(None, n, 8, *([None] * 7)),
        "bjx_smc_reweight": lambda n, m: lib.bjx_smc_reweight(None, n, *([None] * 6)),
        "bjx_smc_log_ess": lambda n, m: lib.bjx_smc_log_ess(None, n, None, None),
        "bjx_smc_ess_solve": lambda n, m: lib.bjx_smc_ess_solve(None, n, None, 0.5, None, None, None, None),
    }
    for name, fn in calls.items():
        assert name in _lib.SIGNATURES
        assert fn(4, 4) != 0 and (name + ": null pointer").encode() in lib.bjx_last_error(), name
        assert fn(-1, 4) != 0 and (name + ": bad sizes").encode() in lib.bjx_last_error(), name  # sizes come first
    for n, m in ((0, 4), (4, -1), ((1 << 24) + 1, 4), (4, (1 << 24) + 1)):
        assert calls["bjx_smc_resample"](n, m) != 0 and b"bjx_smc_resample: bad sizes" in lib.bjx_last_error()
    assert calls["bjx_smc_gather"](0, 4) != 0 and b"bjx_smc_gather: bad sizes" in lib.bjx_last_error()
    assert lib.bjx_smc_gather(None, 4, 4, 0, None, None, None) != 0 and b"bad sizes" in lib.bjx_last_error()
    assert lib.bjx_smc_temper(None, 4, 0, *([None] * 7)) != 0 and b"bjx_smc_temper: bad sizes" in lib.bjx_last_error()
    for target in (0.0, 1.5):
        assert lib.bjx_smc_ess_solve(None, 4, None, target, None, None, None, None) != 0
        assert b"bjx_smc_ess_solve: bad sizes" in lib.bjx_last_error()
    # empty launches are no-ops that need no pointers
    assert lib.bjx_smc_resample(None, 1, 2, 0, 4, 0, None, None, None) == 0
    assert lib.bjx_smc_gather(None, 4, 0, 8, None, None, None) == 0
    assert lib.bjx_smc_temper(None, 0, 8, *([None] * 7)) == 0


def test_restatement_resampling_properties():
    """The fixed-point search is searchsorted(cumsum(w), (i + u) / M) wherever fp64 resolves it: ancestors are
    non-decreasing, inside [0, N), never a particle of weight 0, and a particle of weight w is drawn floor(M w) or
    ceil(M w) times by the systematic scheme."""
    rng = np.random.default_rng(0)
    for n, m in ((1, 5), (7, 7), (1000, 1000), (1000, 333), (333, 1000)):
        w = rng.random(n).astype(f32) ** 3
        w[rng.random(n) < 0.2] = 0
        w[0] = 0 if n > 1 else 1
        w = (w / w.astype(np.float64).sum()).astype(f32)
        for scheme in (rsmc.systematic, rsmc.stratified):
            a = scheme(prng.key(n + m), w, m)
            assert a.dtype == np.int32 and a.shape == (m,) and a.min() >= 0 and a.max() < n
            assert np.all(np.diff(a) >= 0) and np.all(w[a] > 0)
        counts = np.bincount(rsmc.systematic(prng.key(3), w, m), minlength=n)
        assert np.all(np.abs(counts - m * w.astype(np.float64)) < 1.0 + 1e-3)


def test_restatement_solver_and_reweight():
    rng = np.random.default_rng(1)
    ll = (-4.0 * rng.standard_normal(1000) ** 2).astype(f32)
    delta, whole = rsmc.solve_delta(ll, 0.5, f32(1.0))
    assert not whole and 0 < delta < 1
    ess = np.exp(np.float64(rsmc.log_ess(rsmc.log_weights(delta, ll)))) / ll.size
    assert 0.5 <= ess <= 0.505
    w, inc = rsmc.reweight(ll, f32(0.25), f32(0.25) + delta)
    lw = (f32(f32(0.25) + delta) - f32(0.25)) * ll.astype(np.float64)
    assert abs(w.astype(np.float64).sum() - 1) < 1e-6 and np.isclose(inc, np.log(np.mean(np.exp(lw))), rtol=1e-6)
    # the whole interval: the temperature lands on 1.0 exactly
    d, lam = rsmc.next_temperature(ll * f32(1e-3), 0.5, f32(0.7))
    assert lam == f32(1.0) and d == f32(f32(1.0) - f32(0.7))
    # delta == 0: uniform weights whatever the log-likelihoods; -inf / NaN otherwise weigh nothing
    bad = ll.copy()
    bad[3], bad[5] = -np.inf, np.nan
    w0, inc0 = rsmc.reweight(bad, f32(0.5), f32(0.5))
    assert np.all(w0 == f32(1.0 / ll.size)) and abs(inc0) < 1e-7
    w1, _ = rsmc.reweight(bad, f32(0.5), f32(0.6))
    assert w1[3] == 0 and w1[5] == 0 and abs(w1.astype(np.float64).sum() - 1) < 1e-6


def test_restatement_is_a_correct_sampler_on_a_conjugate_target():
    """Prior N(0, I_4), likelihood N(y | x, 0.25 I), y = 1.5: the evidence is N(y; 0, 1.25 I), the posterior
    N(1.2, 0.2 I).  Adaptive tempered SMC, N = 4 096, target_ess = 0.5, systematic resampling, 5 MALA steps of size
    0.1, 16 seeds.  sum(log_likelihood_increment) of every run is within 5 standard deviations of the analytic log
    evidence, the standard deviation being that of the 16 estimates (observed: 0.039, six temperatures per run,
    MALA acceptance 0.83; recorded as smc_restatement.CONJ_LOGZ_SD for the device test).  A move that targets the
    new temperature, a reweighting with the wrong sign or ancestors drawn from the new weights are off by tenths to
    units.  The weighted posterior mean and variance of every run are within 5 standard errors at the run's ESS,
    and every run ends at lmbda == 1.0 exactly."""
    move = rsmc.mala_move(f32(rsmc.CONJ_MALA_STEP))
    estimates, n_steps = [], []
    for seed in range(16):
        st = rsmc.init(prng.normal(prng.key(100 + seed), (4096, rsmc.CONJ_D)))
        k, total, steps = prng.key(200 + seed), 0.0, 0
        while st.lmbda < 1:
            k, sub = prng.split(k, 2)
            st, info = rsmc.adaptive_step(sub, st, 0.5, rsmc.conj_logprior, rsmc.conj_loglikelihood, move, 5)
            total += float(info.log_likelihood_increment)
            steps += 1
            assert steps < 50
        assert st.lmbda == f32(1.0) and st.lmbda.dtype == f32
        mean, var, ess = rsmc.weighted_moments(st)
        mean_se = np.abs(mean - rsmc.CONJ_POST_MEAN) / np.sqrt(rsmc.CONJ_POST_VAR / ess)
        var_se = np.abs(var - rsmc.CONJ_POST_VAR) / (rsmc.CONJ_POST_VAR * np.sqrt(2.0 / ess))
        assert np.all(mean_se <= 5.0) and np.all(var_se <= 5.0), (seed, mean_se, var_se)
        estimates.append(total)
        n_steps.append(steps)
    estimates = np.asarray(estimates)
    sd = estimates.std(ddof=1)
    print("log Z:", rsmc.CONJ_LOGZ, "estimates:", estimates, "sd:", sd, "temperatures:", n_steps)
    assert np.all(np.abs(estimates - rsmc.CONJ_LOGZ) <= 5.0 * sd), (estimates - rsmc.CONJ_LOGZ, sd)
    assert 0.5 * rsmc.CONJ_LOGZ_SD <= sd <= 2.0 * rsmc.CONJ_LOGZ_SD  # the recorded figure is this test's
