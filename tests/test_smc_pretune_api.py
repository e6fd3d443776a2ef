"""Pretuning (``blackjax_amd.pretuning``, ``blackjax_amd.smc.pretuning``): API surface, C-ABI argument checks,
validation that fires before any launch (no GPU needed) and the NumPy restatement the GPU tests hold the kernels
against (tests/smc_pretune_restatement.py), pinned on its own.

The sampler test judges one run (seed 0) of the restated pretuned adaptive tempered SMC by the rule of
``test_smc_extra_api.py::test_restated_waste_free_is_a_correct_sampler_on_a_conjugate_target``: log Z and the weighted
posterior mean within five standard deviations of the ``update_and_take_last`` sampler's spread recorded in that file's
docstring (N = 2048, target_ess = 0.5, systematic resampling, 3 MALA moves per temperature)."""
import inspect

import numpy as np
import pytest

import smc_pretune_restatement as rp
import smc_restatement as rsmc
from oracle import prng, targets as otargets

f32, f64 = np.float32, np.float64

# test_smc_extra_api.py's docstring: the spread of update_and_take_last over 20 seeds at these settings
TAKE_LAST_LOGZ_SD = 0.059
TAKE_LAST_MEAN_SD = np.array([0.0093, 0.0128, 0.0115, 0.0089])
RUN_N, RUN_MOVES, RUN_ALPHA, RUN_SIGMA = 2048, 3, 0.01, 0.1


def test_pretuning_api_surface():
    import blackjax_amd as bjx
    from blackjax_amd import smc

    pt = smc.pretuning
    assert "pretuning" in bjx.__all__ and isinstance(bjx.pretuning, bjx.GenerateSamplingAPI)
    assert "pretuning" in smc.__all__
    assert bjx.pretuning.init is pt.init and bjx.pretuning.build_kernel is pt.build_kernel
    assert bjx.pretuning.differentiable is pt.as_top_level_api
    for name in ("SMCInfoWithParameterDistribution", "esjd", "update_parameter_distribution",
                 "default_measure_factory", "build_pretune", "init", "build_kernel", "as_top_level_api"):
        assert name in pt.__all__ and hasattr(pt, name)
    assert pt.SMCInfoWithParameterDistribution._fields == ("smc_info", "parameter_override")
    assert pt.StateWithParameterOverride is smc.inner_kernel_tuning.StateWithParameterOverride
    assert list(inspect.signature(pt.esjd).parameters) == ["inverse_mass_matrix"]
    sig = inspect.signature(pt.update_parameter_distribution)
    assert list(sig.parameters) == ["key", "previous_param_samples", "previous_particles", "latest_particles",
                                    "measure_of_chain_mixing", "alpha", "sigma_parameters",
                                    "acceptance_probability", "positive_parameters"]
    assert sig.parameters["positive_parameters"].default == ()
    sig = inspect.signature(pt.build_pretune)
    assert list(sig.parameters) == ["mcmc_init_fn", "mcmc_step_fn", "alpha", "sigma_parameters", "n_particles",
                                    "performance_of_chain_measure_factory", "positive_parameters"]
    assert sig.parameters["performance_of_chain_measure_factory"].default is pt.default_measure_factory
    assert sig.parameters["positive_parameters"].default is None
    assert list(inspect.signature(pt.init).parameters) == ["alg_init_fn", "position", "initial_parameter_value"]
    head = ["smc_algorithm", "logprior_fn", "loglikelihood_fn", "mcmc_step_fn", "mcmc_init_fn", "resampling_fn"]
    sig = inspect.signature(pt.build_kernel)
    assert list(sig.parameters) == head + ["pretune_fn", "num_mcmc_steps", "update_strategy", "extra_parameters"]
    assert sig.parameters["num_mcmc_steps"].default == 10
    assert sig.parameters["update_strategy"].default is smc.base.update_and_take_last
    sig = inspect.signature(pt.as_top_level_api)
    assert list(sig.parameters) == head + ["initial_parameter_value", "pretune_fn", "num_mcmc_steps",
                                           "update_strategy", "extra_parameters"]
    assert sig.parameters["extra_parameters"].kind is inspect.Parameter.VAR_KEYWORD
    # the deliberate deviation is written down, and nothing lists pretuning as missing any more
    assert "multinomial" in pt.update_parameter_distribution.__doc__
    assert "choice" in pt.update_parameter_distribution.__doc__
    for mod in (smc, smc.tempered, smc.inner_kernel_tuning):
        scope = mod.__doc__[mod.__doc__.index("Out of scope"):]
        assert "partial" in scope and "pretuning" not in scope.split(".")[0]


def test_pretune_entry_points_reject_bad_arguments_without_gpu():
    from blackjax_amd import _lib

    lib = _lib.load()
    assert lib.bjx_abi_version() == 7
    big_n, big_d = (1 << 24) + 1, (1 << 20) + 1
    for n, d, stride in ((0, 4, 0), (4, 0, 0), (big_n, 4, 0), (4, big_d, 0), (4, 4, 1), (4, 4, -4)):
        assert lib.bjx_smc_esjd(None, n, d, None, None, None, None, stride, None) != 0
        assert b"bjx_smc_esjd: bad sizes" in lib.bjx_last_error()
    for stride in (0, 4):
        assert lib.bjx_smc_esjd(None, 4, 4, None, None, None, None, stride, None) != 0
        assert b"bjx_smc_esjd: null pointer" in lib.bjx_last_error()

    for n, alpha in ((0, 0.1), (big_n, 0.1), (4, -0.1), (4, float("inf")), (4, float("nan"))):
        assert lib.bjx_smc_pretune_weights(None, n, alpha, None, None) != 0
        assert b"bjx_smc_pretune_weights: bad sizes" in lib.bjx_last_error()
    for alpha in (0.0, 0.1):
        assert lib.bjx_smc_pretune_weights(None, 4, alpha, None, None) != 0
        assert b"bjx_smc_pretune_weights: null pointer" in lib.bjx_last_error()

    for n, m, k, stride, log_space in ((0, 4, 4, 0, 0), (4, 0, 4, 0, 0), (4, 4, 0, 0, 0), (big_n, 4, 4, 0, 0),
                                       (4, big_n, 4, 0, 0), (4, 4, big_d, 0, 0), (4, 4, 4, 2, 0), (4, 4, 4, 0, 2)):
        assert lib.bjx_smc_jitter_gather(None, 1, 2, n, m, k, None, None, None, stride, log_space, None) != 0
        assert b"bjx_smc_jitter_gather: bad sizes" in lib.bjx_last_error()
    for k in (1, 3, 4):
        for log_space in (0, 1):
            assert lib.bjx_smc_jitter_gather(None, 1, 2, 4, 4, k, None, None, None, 1, log_space, None) != 0
            assert b"bjx_smc_jitter_gather: null pointer" in lib.bjx_last_error()
    for name in ("bjx_smc_esjd", "bjx_smc_pretune_weights", "bjx_smc_jitter_gather"):
        assert name in _lib.SIGNATURES


def test_validation_before_any_launch():
    import torch

    import blackjax_amd as bjx
    from blackjax_amd import smc

    pt = smc.pretuning
    mala_step, mala_init = bjx.mala.build_kernel(), bjx.mala.init
    # a move whose info has no acceptance_rate is refused when the pretune is built
    with pytest.raises(TypeError, match="acceptance_rate"):
        pt.build_pretune(bjx.orbital_hmc.init, bjx.orbital_hmc.build_kernel(), 0.1, {"step_size": 0.1}, 8)
    for alpha in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            pt.build_pretune(mala_init, mala_step, alpha, {"step_size": 0.1}, 8)
    with pytest.raises(ValueError):
        pt.build_pretune(mala_init, mala_step, 0.1, {}, 8)  # nothing is sampled
    with pytest.raises(ValueError):
        pt.build_pretune(mala_init, mala_step, 0.1, {"step_size": 0.1}, 0)
    with pytest.raises(ValueError):
        pt.build_pretune(mala_init, mala_step, 0.1, {"step_size": 0.1}, 8, positive_parameters=("scale",))
    pretune = pt.build_pretune(mala_init, mala_step, 0.1, {"step_size": 0.1}, 8, positive_parameters=("step_size",))
    assert callable(pretune)
    for step_fn in (bjx.hmc.build_kernel(), bjx.nuts.build_kernel(), bjx.barker.build_kernel()):
        assert pt._info_has_acceptance_rate(step_fn) is True
    assert pt._info_has_acceptance_rate(lambda *a, **k: None) is None  # a user's move: told at the first call

    def logprior(q):
        return -0.5 * (q * q).sum(-1)

    args = (logprior, logprior, mala_step, mala_init, smc.resampling.systematic)
    for bad in (bjx.persistent_sampling_smc, bjx.mala, object()):
        with pytest.raises(TypeError):
            bjx.pretuning(bad, *args, {"step_size": torch.ones(8)}, pretune)
    with pytest.raises(TypeError):
        bjx.pretuning(bjx.adaptive_tempered_smc, *args, {"step_size": torch.ones(8)}, pretune)  # no target_ess
    with pytest.raises(TypeError):
        bjx.pretuning(bjx.tempered_smc, *args, {"step_size": torch.ones(8)}, pretune, target_ess=0.5)
    with pytest.raises(TypeError):
        bjx.pretuning(bjx.tempered_smc, *args, {"step_size": torch.ones(8)}, None)  # pretune_fn is not callable
    alg = bjx.pretuning(bjx.adaptive_tempered_smc, *args, {"step_size": torch.ones(8)}, pretune, target_ess=0.5,
                        num_mcmc_steps=2)
    assert isinstance(alg, bjx.SamplingAlgorithm)
    k = bjx.pretuning.build_kernel(bjx.tempered_smc, *args, pretune)
    assert isinstance(k.tempered_logdensity, smc.tempered.TemperedLogDensity)

    # host tensors, wrong shapes and wrong types are refused by the Python layer: nothing is launched
    key = prng.key(1)
    with pytest.raises(RuntimeError):
        pt.esjd(None)(torch.zeros(8, 3), torch.zeros(8, 3), torch.ones(8))  # there is no CPU fallback
    with pytest.raises(RuntimeError):
        pt.pretune_weights(torch.ones(8), 0.1)
    with pytest.raises(RuntimeError):
        pt.jitter_gather(key, torch.ones(8), torch.zeros(8, dtype=torch.int32), 0.1)
    with pytest.raises(ValueError):
        pt.update_parameter_distribution(key, {"step_size": torch.ones(8)}, torch.zeros(8, 3), torch.zeros(8, 3),
                                         pt.esjd(None), 0.1, {}, torch.ones(8))  # no sigma for a sampled entry
    with pytest.raises(TypeError):
        pt.esjd(None)("x", torch.zeros(8, 3), torch.ones(8))


def test_restated_kernels_properties():
    rng = np.random.default_rng(0)
    n, d = 37, 5
    prev, nxt = rng.standard_normal((n, d)).astype(f32), rng.standard_normal((n, d)).astype(f32)
    acc = rng.random(n).astype(f32)
    m = rp.esjd(prev, nxt, acc)
    np.testing.assert_allclose(m, acc * ((prev - nxt).astype(f64) ** 2).sum(1), rtol=1e-6)
    imm = (0.5 + rng.random((n, d))).astype(f32)
    np.testing.assert_allclose(rp.esjd(prev, nxt, acc, imm), acc * ((prev - nxt).astype(f64) ** 2 / imm).sum(1),
                               rtol=1e-6)
    np.testing.assert_allclose(rp.esjd(prev, nxt, acc, imm[0]), rp.esjd(prev, nxt, acc, np.tile(imm[0], (n, 1))))
    dense = np.diag(imm[0].astype(f64)).astype(f32)
    np.testing.assert_allclose(rp.esjd_dense64(prev, nxt, acc, dense), rp.esjd(prev, nxt, acc, imm[0]), rtol=1e-6)
    # a zero, NaN or negative acceptance rate and a position row holding inf all score exactly 0
    acc2, prev2 = acc.copy(), prev.copy()
    acc2[[0, 1, 2]] = [0.0, np.nan, -0.5]
    prev2[3, 1], prev2[4, 0] = np.inf, np.nan
    m2 = rp.esjd(prev2, nxt, acc2)
    assert np.all(m2[:5] == 0) and np.array_equal(m2[5:], m[5:]) and np.all(np.isfinite(m2))

    for alpha in (0.0, 0.1, 3.0):
        w = rp.pretune_weights(m2, alpha)
        assert w.dtype == f32 and abs(float(w.astype(f64).sum()) - 1.0) <= 1e-6 and np.all(w >= 0)
        assert np.all(w[:5] == w[0]) and (alpha > 0) == bool(w[0] > 0)
    for k in (1, 5, 1025):  # alpha 0 and nothing moved: uniform
        assert np.array_equal(rp.pretune_weights(np.zeros(k, f32), 0.0), np.full(k, f32(1.0 / k), f32))
    np.testing.assert_allclose(rp.pretune_weights(np.zeros(7, f32), 0.3), np.full(7, 1.0 / 7), rtol=1e-7)

    # the noise is the source row's; log space keeps the sign whatever the noise is
    p = rng.standard_normal((n, 3)).astype(f32)
    anc = np.array([0, 0, 5, n - 1, -3, n + 4], np.int32)
    key = prng.key(5)
    z = prng.normal(key, (n, 3))
    out = rp.jitter_gather(key, p, anc, 0.5)
    clipped = np.clip(anc, 0, n - 1)
    np.testing.assert_allclose(out, (p + f32(0.5) * z)[clipped], rtol=1e-6, atol=1e-7)
    assert np.array_equal(out[0], out[1])
    log = rp.jitter_gather(key, p, anc, np.array([0.5, 3.0, 40.0], f32), log_space=True)
    assert np.array_equal(np.signbit(log), np.signbit(p[clipped])) and not np.isnan(log).any()  # (0 and inf included)
    assert np.all(np.isfinite(log[:, 0]) & (log[:, 0] != 0))
    v = rp.jitter_gather(key, p[:, 0], anc, 0.5)
    assert v.shape == (6,) and np.array_equal(v, (p[:, 0] + f32(0.5) * prng.normal(key, (n, 1))[:, 0])[clipped])


def test_restated_pretune_keys_and_passthrough():
    """The trial uses split(split(key, N)[i], 1)[0]; sampled entries are replaced, every other entry is the same
    object; the new rows are the jittered rows of the ancestors drawn with split(key, 2)[1]."""
    ivp, ivl, x0, override, sigma = rp.step_case("hmc")
    prior, lik = otargets.diag_gaussian(ivp), otargets.diag_gaussian(ivl)
    fn = rsmc.tempered_logdensity(prior, lik, f32(0.3))
    key = prng.key(rp.CASE_KEYS["hmc"][0])
    new, (moved, acc, measure, weights, ancestors) = rp.pretune(key, x0, override, fn, rp.make_move("hmc", rp.CASE_L),
                                                                rp.CASE_ALPHA, sigma, rp.CASE_POSITIVE["hmc"])
    assert new["num_integration_steps"] is override["num_integration_steps"] and set(new) == set(override)
    move = rp.make_move("hmc", rp.CASE_L)(override)
    st, info = move.step(prng.split(prng.split(key, rp.CASE_N), 1)[:, 0], move.init(x0, fn), fn)
    assert np.array_equal(st.position, moved) and np.array_equal(info.acceptance_rate, acc)
    assert np.array_equal(measure, rp.esjd(x0, moved, acc, override["inverse_mass_matrix"]))
    assert 0 < int(info.is_accepted.sum()) and np.all(np.diff(ancestors) >= 0)
    keys = prng.split(key, 2)
    for name in sigma:
        assert new[name].shape == override[name].shape and np.all(new[name] > 0)
        assert np.array_equal(new[name], rp.jitter_gather(keys[0], override[name], ancestors, sigma[name], True))


@pytest.mark.parametrize("inner", ["mala", "hmc"])
def test_case_keys_leave_no_ancestor_near_a_boundary(inner):
    """The keys of the GPU full-step tests: in the restatement alone, no threshold of the parameter resampling lies
    within 2^-20 (relative) of a cumulative-weight boundary, so the GPU test leaves nothing out for them."""
    ivp, ivl, x0, override, sigma = rp.step_case(inner)
    prior, lik = otargets.diag_gaussian(ivp), otargets.diag_gaussian(ivl)
    move_of = rp.make_move(inner, rp.CASE_L)
    st = rsmc.init(x0)
    k_pretune, k_fixed, k_adaptive = (prng.key(s) for s in rp.CASE_KEYS[inner])
    # the lone pretune call is made at temperature CASE_LMBDA, both steps start from the initial state
    cases = [(k_pretune, rp.CASE_LMBDA), (prng.split(k_fixed, 2)[1], st.lmbda),
             (prng.split(k_adaptive, 2)[1], st.lmbda)]
    for key, lam in cases:
        fn = rsmc.tempered_logdensity(prior, lik, lam)
        _, (_, _, _, weights, ancestors) = rp.pretune(key, st.particles, override, fn, move_of, rp.CASE_ALPHA, sigma,
                                                      rp.CASE_POSITIVE[inner])
        near = rp.near_boundary(prng.split(key, 2)[1], weights)
        assert not near.any(), (inner, int(near.sum()))
        assert len(np.unique(ancestors)) < rp.CASE_N  # a parameter row was duplicated and one dropped


def _run(seed):
    st = rsmc.init(prng.normal(prng.key(100 + seed), (RUN_N, rsmc.CONJ_D)))
    u = prng.uniform(prng.key(300 + seed), (RUN_N,)).astype(f64)
    step0 = (10.0 ** (-3.0 + 3.0 * u)).astype(f32)  # log-uniform over [1e-3, 1]
    override = {"step_size": step0}
    k, total, steps = prng.key(200 + seed), 0.0, 0
    while st.lmbda < 1:
        k, sub = prng.split(k, 2)
        st, override, info = rp.pretuned_step(sub, st, override, None, rsmc.conj_logprior, rsmc.conj_loglikelihood,
                                              rp.make_move("mala"), RUN_MOVES, RUN_ALPHA, {"step_size": RUN_SIGMA},
                                              ("step_size",), rsmc.systematic, 0.5)
        total += float(info.log_likelihood_increment)
        steps += 1
        assert steps < 50
    assert st.lmbda == f32(1.0)
    return total, rsmc.weighted_moments(st)[0], step0, override["step_size"], steps


def test_restated_pretuned_smc_is_a_correct_sampler_on_a_conjugate_target():
    """Step sizes start log-uniform over three decades, [1e-3, 1].  Measured at seed 0: 6 temperatures, log Z off by
    0.0096, the mean by at most 0.0115; the median step size ends at 0.352 (MALA's hand-tuned 0.1 accepts more but
    jumps less), inside the initial range [0.0010, 0.9991]: with sigma = 0.1 in log space, six jitters alone move a
    value by a factor of exp(0.1 sqrt 6) = 1.28, so the population got there by selection."""
    log_z, mean, step0, step1, steps = _run(0)
    print("log Z", log_z, "analytic", rsmc.CONJ_LOGZ, "mean", mean, "analytic", rsmc.CONJ_POST_MEAN, "temperatures",
          steps, "median step size", np.median(step1), "initial range", step0.min(), step0.max())
    assert abs(log_z - rsmc.CONJ_LOGZ) <= 5.0 * TAKE_LAST_LOGZ_SD
    assert np.all(np.abs(mean - rsmc.CONJ_POST_MEAN) <= 5.0 * TAKE_LAST_MEAN_SD)
    assert step0.min() <= np.median(step1) <= step0.max()
    assert np.all(step1 > 0)
