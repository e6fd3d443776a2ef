"""``blackjax_amd.persistent_sampling_smc`` / ``adaptive_persistent_sampling_smc``: API surface, C-ABI argument checks
(no GPU needed) and the NumPy restatement the GPU tests hold the kernels against
(tests/persistent_smc_restatement.py), pinned on its own as a sampler."""
import numpy as np
import pytest

import persistent_smc_restatement as rps
import smc_restatement as rsmc
from oracle import prng

f32 = np.float32


def test_persistent_smc_api_surface():
    import blackjax_amd as bjx
    from blackjax_amd import smc

    for name in ("persistent_sampling_smc", "adaptive_persistent_sampling_smc"):
        assert name in bjx.__all__ and isinstance(getattr(bjx, name), bjx.GenerateSamplingAPI)
    for name in ("persistent_sampling", "adaptive_persistent_sampling"):
        assert name in smc.__all__
    ps, aps = smc.persistent_sampling, smc.adaptive_persistent_sampling
    assert bjx.persistent_sampling_smc.init is ps.init and bjx.persistent_sampling_smc.build_kernel is ps.build_kernel
    assert bjx.adaptive_persistent_sampling_smc.init is aps.init is ps.init
    assert bjx.adaptive_persistent_sampling_smc.build_kernel is aps.build_kernel
    fields = ("persistent_particles", "persistent_log_likelihoods", "persistent_log_Z", "tempering_schedule",
              "iteration")
    assert ps.PersistentSMCState._fields == fields == rps.PersistentSMCState._fields
    assert ps.PersistentStateInfo._fields == ("ancestors", "update_info") == rps.PersistentStateInfo._fields
    for prop in ("particles", "log_likelihoods", "log_Z", "tempering_param", "n_particles", "persistent_weights"):
        assert isinstance(getattr(ps.PersistentSMCState, prop), property), prop
    for f in (ps.init, ps.remove_padding, ps.compute_log_Z, ps.compute_log_persistent_weights,
              ps.compute_persistent_weights, ps.resample_from_persistent, ps.step, ps.build_kernel,
              ps.as_top_level_api, aps.calculate_lambda, aps.build_kernel, aps.as_top_level_api):
        assert callable(f)

    def logprior(q):
        return -0.5 * (q * q).sum(-1)

    def loglik(q):
        return -2.0 * ((q - 1.5) ** 2).sum(-1)

    params = {"step_size": 0.1}
    fixed = bjx.persistent_sampling_smc(logprior, loglik, 8, bjx.mala.build_kernel(), bjx.mala.init, params,
                                        smc.resampling.systematic, num_mcmc_steps=3)
    adaptive = bjx.adaptive_persistent_sampling_smc(logprior, loglik, 8, bjx.mala.build_kernel(), bjx.mala.init,
                                                    params, smc.resampling.stratified, 2.0)
    for alg in (fixed, adaptive):
        assert isinstance(alg, bjx.SamplingAlgorithm) and callable(alg.init) and callable(alg.step)
    k = aps.build_kernel(logprior, loglik, bjx.mala.build_kernel(), bjx.mala.init, smc.resampling.systematic, 0.9)
    assert isinstance(k.tempered_logdensity, smc.tempered.TemperedLogDensity)
    # construction-time refusals
    with pytest.raises(ValueError):
        bjx.persistent_sampling_smc(logprior, loglik, 0, bjx.mala.build_kernel(), bjx.mala.init, params,
                                    smc.resampling.systematic)
    for bad in (0.0, -0.5):
        with pytest.raises(ValueError):
            bjx.adaptive_persistent_sampling_smc(logprior, loglik, 8, bjx.mala.build_kernel(), bjx.mala.init, params,
                                                 smc.resampling.systematic, bad)


def test_persistent_tile_and_workspace_without_gpu():
    from blackjax_amd import _lib
    from blackjax_amd.smc import persistent_sampling

    lib = _lib.load()
    T = lib.bjx_smc_persistent_tile()
    assert T == persistent_sampling.REDUCTION_TILE
    ws = lib.bjx_smc_persistent_workspace_bytes
    assert "bjx_smc_persistent_workspace_bytes" in _lib.INT64_FUNCTIONS
    assert ws(0) == 0 and ws(-1) == 0 and ws((1 << 24) + 1) == 0
    head = ws(1) - 24  # one tile triple of three doubles after the head
    assert head >= 0 and ws(T) == head + 24 and ws(T + 1) == head + 48 and ws(1 << 24) == head + 24 * ((1 << 24) // T)
    assert ws(1) % 8 == 0


def test_persistent_entry_points_reject_bad_arguments_without_gpu():
    from blackjax_amd import _lib

    lib = _lib.load()
    calls = {
        "bjx_smc_persistent_denominator": lambda p: lib.bjx_smc_persistent_denominator(None, p, 3, *([None] * 4)),
        "bjx_smc_persistent_weights": lambda p: lib.bjx_smc_persistent_weights(None, p, *([None] * 7)),
        "bjx_smc_persistent_ess_solve": lambda p: lib.bjx_smc_persistent_ess_solve(None, p, None, None, 8.0, None,
                                                                                   None, None, None),
    }
    for name, fn in calls.items():
        assert name in _lib.SIGNATURES
        assert fn(4) != 0 and (name + ": null pointer").encode() in lib.bjx_last_error(), name
        for p in (-1, (1 << 24) + 1):  # sizes come first
            assert fn(p) != 0 and (name + ": bad sizes").encode() in lib.bjx_last_error(), (name, p)
    assert "bjx_smc_persistent_tile" in _lib.SIGNATURES
    assert lib.bjx_smc_persistent_denominator(None, 4, 0, *([None] * 4)) != 0  # no mixture term
    assert b"bjx_smc_persistent_denominator: bad sizes" in lib.bjx_last_error()
    for p in (0,):
        assert calls["bjx_smc_persistent_weights"](p) != 0 and b"weights: bad sizes" in lib.bjx_last_error()
        assert calls["bjx_smc_persistent_ess_solve"](p) != 0 and b"ess_solve: bad sizes" in lib.bjx_last_error()
    for target in (0.0, -1.0, float("nan")):
        assert lib.bjx_smc_persistent_ess_solve(None, 4, None, None, target, None, None, None, None) != 0
        assert b"bjx_smc_persistent_ess_solve: bad sizes" in lib.bjx_last_error()
    # an empty launch is a no-op that needs no pointers
    assert lib.bjx_smc_persistent_denominator(None, 0, 3, *([None] * 4)) == 0


def test_first_iteration_is_the_tempered_reweighting():
    """At i = 1 the mixture is the prior alone: den = 0, lw = lam * ll, logZ_1 = log mean exp -- the arithmetic of
    smc_restatement.reweight from temperature 0."""
    rng = np.random.default_rng(3)
    ll = (-4.0 * rng.standard_normal(1000) ** 2).astype(f32)
    ll[7], ll[11] = -np.inf, np.nan
    den = rps.denominator(ll, np.zeros(1, f32), np.zeros(1, f32))
    assert np.array_equal(den, np.zeros(1000, f32))  # 0 * ll = 0, whatever ll is
    for lam in (0.05, 0.6, 1.0):
        log_w, w, log_z, _ = rps.weigh(f32(lam), ll, den)
        w_r, inc_r = rsmc.reweight(ll, f32(0.0), f32(lam))
        np.testing.assert_allclose(w, w_r, rtol=0, atol=1e-6)
        assert abs(float(log_z) - float(inc_r)) <= 1e-6 and w[7] == 0 and w[11] == 0
        assert log_w[7] == -np.inf and abs(np.exp(log_w.astype(np.float64)).sum() - 1) < 1e-6


def _run(seed, target_ess, max_iterations=24):
    move = rsmc.mala_move(f32(rsmc.CONJ_MALA_STEP))
    st = rps.init(prng.normal(prng.key(100 + seed), (4096, rsmc.CONJ_D)), rsmc.conj_loglikelihood, max_iterations)
    k, lams = prng.key(200 + seed), []
    while st.tempering_param < 1:
        k, sub = prng.split(k, 2)
        st, _ = rps.adaptive_step(sub, st, target_ess, rsmc.conj_logprior, rsmc.conj_loglikelihood, move, 5)
        lams.append(st.tempering_param)
    return st, lams


def test_restatement_is_a_correct_sampler_on_a_conjugate_target():
    """The conjugate case of test_smc_api.py (evidence N(y; 0, 1.25 I), posterior N(1.2, 0.2 I)) under adaptive
    persistent sampling: N = 4 096, target_ess = 0.9, systematic resampling, 5 MALA steps of size 0.1, 16 seeds.
    ``log_Z`` of every run is within 5 standard deviations of the analytic log evidence, the standard deviation being
    that of the 16 estimates (recorded as persistent_smc_restatement.PS_CONJ_LOGZ_SD for the device test), the mean and
    variance under ``persistent_weights`` are within 5 standard errors at the run's ESS, and every run ends at
    exactly 1.0."""
    estimates, n_steps, esses = [], [], []
    for seed in range(16):
        st, lams = _run(seed, 0.9)
        assert st.tempering_param == f32(1.0) and st.tempering_param.dtype == f32
        assert all(b > a for a, b in zip([0.0] + lams, lams))
        mean, var, ess = rps.persistent_moments(st)
        mean_se = np.abs(mean - rsmc.CONJ_POST_MEAN) / np.sqrt(rsmc.CONJ_POST_VAR / ess)
        var_se = np.abs(var - rsmc.CONJ_POST_VAR) / (rsmc.CONJ_POST_VAR * np.sqrt(2.0 / ess))
        assert np.all(mean_se <= 5.0) and np.all(var_se <= 5.0), (seed, mean_se, var_se)
        estimates.append(float(st.log_Z))
        n_steps.append(st.iteration)
        esses.append(ess)
    estimates = np.asarray(estimates)
    sd = estimates.std(ddof=1)
    print("log Z:", rsmc.CONJ_LOGZ, "estimates:", estimates, "sd:", sd, "iterations:", n_steps, "ESS:", esses)
    assert np.all(np.abs(estimates - rsmc.CONJ_LOGZ) <= 5.0 * sd), (estimates - rsmc.CONJ_LOGZ, sd)
    assert 0.5 * rps.PS_CONJ_LOGZ_SD <= sd <= 2.0 * rps.PS_CONJ_LOGZ_SD  # the recorded figure is this test's
    assert min(esses) > 4096  # the persistent set holds more effective particles than one iteration has


def test_a_target_above_the_reachable_ess_does_not_move_the_temperature():
    """target_ess = 2: N particles cannot hold 2 N effective ones, so the first step returns delta == 0 bit for bit
    and adds a slot at temperature 0; the run still ends at exactly 1.0 within 16 iterations."""
    st0 = rps.init(prng.normal(prng.key(100), (4096, rsmc.CONJ_D)), rsmc.conj_loglikelihood, 16)
    delta, lam = rps.calculate_lambda(st0, 2.0)
    assert delta.dtype == f32 and delta.view(np.uint32) == 0 and lam.view(np.uint32) == 0
    st, lams = _run(0, 2.0, max_iterations=16)
    print("temperatures:", lams)
    assert lams[0] == 0 and st.tempering_param == f32(1.0) and st.iteration <= 16
    assert all(b >= a for a, b in zip(lams, lams[1:]))
