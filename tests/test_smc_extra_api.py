"""Multinomial / residual resampling, waste-free SMC, inner-kernel tuning and ``smc.tuning``: API surface, C-ABI
argument checks (no GPU needed) and the NumPy restatement the GPU tests hold the kernels against
(tests/smc_extra_restatement.py), pinned on its own.

The spread the waste-free sampler test uses (``python tests/test_smc_extra_api.py`` prints it): adaptive tempered SMC
on smc_restatement's conjugate target, N = 2048, target_ess = 0.5, systematic resampling, MALA steps of size 0.1,
``update_and_take_last`` with ``num_mcmc_steps = p - 1 = 3``, seeds 0 .. 19 (particles ``key(100 + seed)``, run
``key(200 + seed)``): standard deviation of log Z 0.059, of the weighted posterior mean per coordinate
0.0093, 0.0128, 0.0115, 0.0089.  The waste-free sampler (p = 4, so M = 512 chains of 3 transitions) at seed 0 is off
by 0.161 in log Z and by at most 0.038 in the mean.  Its own spread over the same 20 seeds is 0.171 in log Z -- a
waste-free run makes a quarter of the gradient evaluations of the run it is compared with -- and seeds 4, 6 and 16
of the 20 miss the 5 x 0.059 bound (0.314, 0.302, 0.305); the test runs seed 0."""
import inspect

import numpy as np
import pytest

import smc_extra_restatement as rx
import smc_restatement as rsmc
from oracle import prng

f32, f64 = np.float32, np.float64

WF_N, WF_P = 2048, 4
TAKE_LAST_LOGZ_SD = 0.059
TAKE_LAST_MEAN_SD = np.array([0.0093, 0.0128, 0.0115, 0.0089])


def _gamma_weights(n, seed=0):
    """gamma(0.5) weights, every fifth one zero."""
    w = np.random.default_rng(seed).gamma(0.5, size=n)
    w[::5] = 0.0
    if n < 5:
        w[-1] = max(w[-1], 0.5)
    return (w / w.sum()).astype(f32)


def test_extra_api_surface():
    import blackjax_amd as bjx
    from blackjax_amd import smc

    assert "inner_kernel_tuning" in bjx.__all__ and isinstance(bjx.inner_kernel_tuning, bjx.GenerateSamplingAPI)
    for name in ("waste_free", "inner_kernel_tuning", "tuning", "waste_free_smc"):
        assert name in smc.__all__ and hasattr(smc, name)
    for name in ("multinomial", "residual", "systematic", "stratified"):
        fn = getattr(smc.resampling, name)
        assert name in smc.resampling.__all__ and callable(fn._bjx_trusted)
        assert list(inspect.signature(fn).parameters) == ["rng_key", "weights", "num_samples"]
    ikt = smc.inner_kernel_tuning
    assert bjx.inner_kernel_tuning.init is ikt.init and bjx.inner_kernel_tuning.build_kernel is ikt.build_kernel
    assert ikt.StateWithParameterOverride._fields == ("sampler_state", "parameter_override")
    assert list(inspect.signature(ikt.init).parameters) == ["alg_init_fn", "position", "initial_parameter_value"]
    head = ["smc_algorithm", "logprior_fn", "loglikelihood_fn", "mcmc_step_fn", "mcmc_init_fn", "resampling_fn",
            "mcmc_parameter_update_fn"]
    sig = inspect.signature(ikt.build_kernel)
    assert list(sig.parameters) == head + ["num_mcmc_steps", "extra_parameters"]
    assert sig.parameters["num_mcmc_steps"].default == 10
    sig = inspect.signature(ikt.as_top_level_api)
    assert list(sig.parameters) == head + ["initial_parameter_value", "num_mcmc_steps", "extra_parameters"]
    assert sig.parameters["num_mcmc_steps"].default == 10
    assert sig.parameters["extra_parameters"].kind is inspect.Parameter.VAR_KEYWORD
    for mod in (smc.tempered, smc.adaptive_tempered):
        for fn in (mod.as_top_level_api, mod.build_kernel):
            last = list(inspect.signature(fn).parameters.values())[-1]
            assert last.name == "update_strategy" and last.default is smc.base.update_and_take_last
    assert list(inspect.signature(smc.waste_free_smc).parameters) == ["n_particles", "p"]
    fp = smc.tuning.from_particles
    for name in ("particles_means", "particles_stds", "particles_covariance_matrix", "mass_matrix_from_particles",
                 "particles_as_rows"):
        assert name in fp.__all__ and list(inspect.signature(getattr(fp, name)).parameters) == ["particles"]
    assert "inverse_mass_matrix" in fp.mass_matrix_from_particles.__doc__
    sig = inspect.signature(smc.tuning.from_kernel_info.update_scale_from_acceptance_rate)
    assert list(sig.parameters) == ["scales", "acceptance_rates", "target_acceptance_rate"]
    assert sig.parameters["target_acceptance_rate"].default == 0.234
    assert "inf" in smc.resampling.multinomial.__doc__  # the deliberate deviation is written down
    # meads' permutation is the shared helper, unchanged
    assert bjx.meads._permutation is bjx.random.permutation
    for seed, n in ((0, 1), (3, 7), (5, 1000)):
        assert np.array_equal(bjx.random.permutation(prng.key(seed), n), prng.permutation(prng.key(seed), n))


def test_validation_without_gpu():
    import torch

    import blackjax_amd as bjx
    from blackjax_amd import smc

    for n, p in ((10, 3), (10, 1), (10, 0), (0, 2)):
        with pytest.raises(ValueError):
            smc.waste_free_smc(n, p)
    strategy = smc.waste_free_smc(12, 3)
    assert strategy.num_resampled == 4
    with pytest.raises(ValueError, match="num_mcmc_steps"):
        strategy(bjx.mala.init, None, bjx.mala.build_kernel(), 5, 12)
    with pytest.raises(ValueError):
        strategy(bjx.mala.init, None, bjx.mala.build_kernel(), None, 16)  # built for another N
    update, m = strategy(bjx.mala.init, None, bjx.mala.build_kernel(), None, 12)
    assert m == 4 and callable(update)

    def logprior(q):
        return -0.5 * (q * q).sum(-1)

    args = (logprior, logprior, bjx.mala.build_kernel(), bjx.mala.init, smc.resampling.systematic,
            lambda key, state, info: {"step_size": 0.1})
    for bad in (bjx.persistent_sampling_smc, bjx.mala, object()):
        with pytest.raises(TypeError):
            bjx.inner_kernel_tuning(bad, *args, {"step_size": 0.1})
    with pytest.raises(TypeError):
        bjx.inner_kernel_tuning(bjx.adaptive_tempered_smc, *args, {"step_size": 0.1})  # no target_ess
    with pytest.raises(TypeError):
        bjx.inner_kernel_tuning(bjx.tempered_smc, *args, {"step_size": 0.1}, target_ess=0.5)
    alg = bjx.inner_kernel_tuning(bjx.adaptive_tempered_smc, *args, {"step_size": 0.1}, target_ess=0.5,
                                  update_strategy=smc.waste_free_smc(8, 2), num_mcmc_steps=None)
    assert isinstance(alg, bjx.SamplingAlgorithm)
    k = bjx.inner_kernel_tuning.build_kernel(bjx.tempered_smc, *args)
    assert isinstance(k.tempered_logdensity, smc.tempered.TemperedLogDensity)

    upd = smc.tuning.from_kernel_info.update_scale_from_acceptance_rate
    with pytest.raises(ValueError):
        upd(torch.ones(3), torch.ones(4))
    scales, rates = np.array([0.5, 1.0, 2.0], f32), np.array([0.1, 0.234, 0.9], f32)
    np.testing.assert_allclose(upd(torch.as_tensor(scales), torch.as_tensor(rates)).numpy(),
                               rx.update_scale_from_acceptance_rate(scales, rates), rtol=1e-6)
    np.testing.assert_allclose(upd(torch.as_tensor(scales), torch.as_tensor(rates), 0.5).numpy(),
                               scales * np.exp(rates.astype(f64) - 0.5), rtol=1e-6)


def test_new_entry_points_reject_bad_arguments_without_gpu():
    from blackjax_amd import _lib
    from blackjax_amd.smc.tuning import from_particles

    lib = _lib.load()
    T = lib.bjx_smc_scan_tile()
    ws = lib.bjx_smc_resample_sorted_workspace_bytes
    assert ws(1, 1) == 8 * (2 * 1 + 2) and ws(T, T - 1) == 8 * (2 * T + T)
    assert ws(T + 1, T) == 8 * (2 * (T + 1 + 2) + (T + 1 + 2))  # every scan above one tile adds its tile sums
    for n, m in ((0, 4), (4, -1), ((1 << 24) + 1, 4), (4, (1 << 24) + 1)):
        assert ws(n, m) == 0
        assert lib.bjx_smc_resample_sorted(None, 1, 2, 0, n, m, None, None, None, None) != 0
        assert b"bjx_smc_resample_sorted: bad sizes" in lib.bjx_last_error()
    assert lib.bjx_smc_resample_sorted(None, 1, 2, 2, 4, 4, None, None, None, None) != 0  # no such mode
    assert b"bjx_smc_resample_sorted: bad sizes" in lib.bjx_last_error()
    for mode in (0, 1):
        assert lib.bjx_smc_resample_sorted(None, 1, 2, mode, 4, 4, None, None, None, None) != 0
        assert b"bjx_smc_resample_sorted: null pointer" in lib.bjx_last_error()
        assert lib.bjx_smc_resample_sorted(None, 1, 2, mode, 4, 0, None, None, None, None) == 0  # an empty launch

    assert lib.bjx_smc_scatter_rows(None, 4, 8, None, 0, 1, None) != 0
    assert b"bjx_smc_scatter_rows: null pointer" in lib.bjx_last_error()
    for m, d, row0, stride in ((-1, 8, 0, 1), (4, 0, 0, 1), (4, 8, -1, 1), (4, 8, 0, 0)):
        assert lib.bjx_smc_scatter_rows(None, m, d, None, row0, stride, None) != 0
        assert b"bjx_smc_scatter_rows: bad sizes" in lib.bjx_last_error()
    assert lib.bjx_smc_scatter_rows(None, 0, 8, None, 0, 1, None) == 0

    R = lib.bjx_smc_moments_tile()
    assert R == from_particles.MOMENTS_TILE
    mws = lib.bjx_smc_particle_moments_workspace_bytes
    assert mws(1, 1) == 8 * 4 and mws(R, 3) == 8 * (2 * 3 + 2 * 3) and mws(R + 1, 3) == 8 * (4 * 3 + 2 * 3)
    for n, d in ((0, 4), (4, 0), ((1 << 24) + 1, 4), (4, (1 << 20) + 1)):
        assert mws(n, d) == 0
        assert lib.bjx_smc_particle_moments(None, n, d, None, None, None, None) != 0
        assert b"bjx_smc_particle_moments: bad sizes" in lib.bjx_last_error()
    assert lib.bjx_smc_particle_moments(None, 4, 4, None, None, None, None) != 0
    assert b"bjx_smc_particle_moments: null pointer" in lib.bjx_last_error()
    for name in ("bjx_smc_resample_sorted", "bjx_smc_scatter_rows", "bjx_smc_particle_moments"):
        assert name in _lib.SIGNATURES


def test_restated_multinomial_properties():
    for n, m in ((1, 5), (7, 7), (1500, 3000)):
        w = _gamma_weights(n)
        a = rx.multinomial(prng.key(n + m), w, m)
        assert a.dtype == np.int32 and a.shape == (m,) and a.min() >= 0 and a.max() < n
        assert np.all(np.diff(a) >= 0) and np.all(w[a] > 0)
    one = np.zeros(64, f32)
    one[17] = 1.0
    assert np.all(rx.multinomial(prng.key(2), one, 33) == 17)
    pos = rx.sorted_uniforms(prng.key(9), 1000)
    assert pos.dtype == f64 and np.all(np.diff(pos) >= 0) and pos[0] >= 0 and pos[-1] <= 1


@pytest.mark.parametrize("n,m", [(64, 16), (1025, 1025)])
def test_restated_multinomial_counts_follow_the_weights(n, m):
    """Over 400 keys the number of draws of particle j is Binomial(400 M, w_j): |z| <= 5 for every particle of
    positive weight, and a particle of weight zero is never drawn."""
    w = _gamma_weights(n)
    keys = 400
    counts = np.zeros(n, np.int64)
    for k in prng.split(prng.key(1234), keys):
        a = rx.multinomial(k, w, m)
        assert np.all(np.diff(a) >= 0)
        counts += np.bincount(a, minlength=n)
    assert np.all(counts[w == 0] == 0)
    p = w.astype(f64) / w.astype(f64).sum()
    ok = w > 0
    z = (counts[ok] - keys * m * p[ok]) / np.sqrt(keys * m * p[ok] * (1 - p[ok]))
    print("n", n, "m", m, "max |z|", np.abs(z).max())
    assert np.abs(z).max() <= 5.0


def test_restated_residual_properties():
    for n, m in ((7, 7), (64, 16), (1500, 3000), (1025, 1025)):
        w = _gamma_weights(n)
        cnt, rem = rx.residual_split(w, m)
        assert np.array_equal(cnt, np.floor(m * w.astype(f64)).astype(np.int64)) and np.all(rem >= 0)
        for seed in range(3):
            a = rx.residual(prng.key(10 * n + seed), w, m)
            assert a.dtype == np.int32 and a.shape == (m,) and a.min() >= 0 and a.max() < n
            counts = np.bincount(a, minlength=n)
            assert np.all(counts >= cnt) and np.all(w[a] > 0)
            s = int(cnt.sum())
            assert np.array_equal(a[:s], np.repeat(np.arange(n), cnt))
    # every M w_j an integer: S == M, nothing is drawn
    m = 64
    k = np.array([0, 5, 1, 0, 30, 8, 20], np.int64)
    w = (k / f64(m)).astype(f32)
    a = rx.residual(prng.key(3), w, m)
    assert np.array_equal(np.bincount(a, minlength=len(k)), k) and np.array_equal(a, np.repeat(np.arange(len(k)), k))


def _run(seed, waste_free):
    move = rsmc.mala_move(f32(rsmc.CONJ_MALA_STEP))
    st = rsmc.init(prng.normal(prng.key(100 + seed), (WF_N, rsmc.CONJ_D)))
    k, total, steps = prng.key(200 + seed), 0.0, 0
    while st.lmbda < 1:
        k, sub = prng.split(k, 2)
        st, info = rx.adaptive_step(sub, st, 0.5, rsmc.conj_logprior, rsmc.conj_loglikelihood, move,
                                    None if waste_free else WF_P - 1, rsmc.systematic, WF_P if waste_free else None)
        assert info.ancestors.shape == ((WF_N // WF_P,) if waste_free else (WF_N,))
        total += float(info.log_likelihood_increment)
        steps += 1
        assert steps < 50
    assert st.lmbda == f32(1.0)
    return total, rsmc.weighted_moments(st)[0]


def test_restated_waste_free_is_a_correct_sampler_on_a_conjugate_target():
    """Log Z and the weighted posterior mean of one waste-free run within five standard deviations of the
    ``update_and_take_last`` sampler's (this file's docstring)."""
    log_z, mean = _run(0, True)
    print("log Z", log_z, "analytic", rsmc.CONJ_LOGZ, "mean", mean, "analytic", rsmc.CONJ_POST_MEAN)
    assert abs(log_z - rsmc.CONJ_LOGZ) <= 5.0 * TAKE_LAST_LOGZ_SD
    assert np.all(np.abs(mean - rsmc.CONJ_POST_MEAN) <= 5.0 * TAKE_LAST_MEAN_SD)


def test_restated_waste_free_layout_and_keys():
    """Rows [0, M) are the resampled particles, row M + i (p - 1) + t is chain i after transition t + 1, and chain i
    at transition t uses split(split(key, M)[i], p - 1)[t]."""
    m, p, d = 5, 3, 2
    x = prng.normal(prng.key(1), (m, d))
    fn = rsmc.tempered_logdensity(rsmc.conj_logprior, rsmc.conj_loglikelihood, f32(0.3))
    move = rsmc.mala_move(f32(0.2))
    out, infos = rx.waste_free_update(prng.key(2), x, fn, move, p)
    assert out.shape == (m * p, d) and len(infos) == p - 1 and np.array_equal(out[:m], x)
    chain_keys = prng.split(prng.key(2), m)
    st = move.init(x, fn)
    for t in range(p - 1):
        st, _ = move.step(prng.split(chain_keys, p - 1)[:, t], st, fn)
        for i in range(m):
            assert np.array_equal(out[m + i * (p - 1) + t], st.position[i])


def test_restated_moments():
    x = (3.0 + 2.0 * np.random.default_rng(0).standard_normal((1000, 3))).astype(f32)
    np.testing.assert_allclose(rx.particles_means(x), x.astype(f64).mean(0), rtol=1e-7)
    np.testing.assert_allclose(rx.particles_stds(x), x.astype(f64).std(0), rtol=1e-7)
    np.testing.assert_allclose(rx.particles_covariance_matrix(x), np.cov(x.astype(f64), rowvar=False), rtol=1e-12)
    assert np.all(rx.particles_stds(x[:1]) == 0)


if __name__ == "__main__":  # the spread this file's docstring records
    runs = [_run(seed, False) for seed in range(20)]
    log_z = np.array([r[0] for r in runs])
    means = np.array([r[1] for r in runs])
    print("update_and_take_last: sd of log Z", log_z.std(ddof=1), "sd of the mean", means.std(axis=0, ddof=1))
    runs = [_run(seed, True) for seed in range(20)]
    print("waste-free: log Z errors", np.array([r[0] for r in runs]) - rsmc.CONJ_LOGZ)
    print("waste-free: largest mean error", [float(np.abs(r[1] - rsmc.CONJ_POST_MEAN).max()) for r in runs])
