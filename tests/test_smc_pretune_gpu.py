"""GPU parity of pretuning (blackjax_amd/smc/pretuning.py, csrc/bjx_smc_pretune.hip, include/bjx_hip.h "SMC") against
the NumPy restatement of the reference's arithmetic, tests/smc_pretune_restatement.py."""
import numpy as np
import pytest
import torch

import blackjax_amd as bjx
import smc_extra_restatement as rx
import smc_pretune_restatement as rp
import smc_restatement as rsmc
from blackjax_amd import metrics, smc
from oracle import prng, targets as otargets

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
pt = smc.pretuning

RTOL, ATOL = 1e-6, 1e-7  # test_smc_gpu.py's: fp64 sums rounded once to fp32
POS_TOL = 1e-6  # test_smc_gpu.py's tolerance (relative and absolute) for a moved particle
DELTA_TOL = 1e-4  # test_smc_gpu.py's: the temperature, as a fraction of the interval searched
# the dense (D, D) measure goes through an fp32 Cholesky factor and an fp32 triangular solve; against the fp64 solve
# the largest relative error measured at D = 65 (N = 257, condition number 3.3) was 1.92e-7: 8 x that
DENSE_RTOL = 8 * 1.92e-7


def t2n(t):
    return t.detach().cpu().numpy()


def dev_t(a, dev):
    return torch.as_tensor(np.asarray(a), device=dev)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.int32)


# ----------------------------------------------------------------------------- esjd
def _esjd_inputs(n, d):
    rng = np.random.default_rng(1000 * n + d)
    prev, nxt = rng.standard_normal((n, d)).astype(f32), rng.standard_normal((n, d)).astype(f32)
    acc = rng.random(n).astype(f32)
    zero_rows = []
    if n >= 7:  # a rejected trial, a NaN acceptance rate, a divergent proposal: all of them score exactly 0
        acc[0], acc[1] = 0.0, np.nan
        prev[2, d // 2] = np.inf
        nxt[3, 0] = np.nan
        zero_rows = [0, 1, 2, 3]
    return prev, nxt, acc, zero_rows, (0.25 + rng.random((n, d))).astype(f32)


# N: one row, less than a workgroup's four, more than one workgroup, one more than a multiple of four.  D: one lane,
# no multiple of 4, exactly one 16-byte piece, a partial second 4-byte sweep, more than one 16-byte piece per lane
@pytest.mark.parametrize("d", [1, 3, 4, 65, 260])
@pytest.mark.parametrize("n", [1, 7, 257, 1025])
def test_esjd_matches_restatement(dev, n, d):
    prev, nxt, acc, zero_rows, imm = _esjd_inputs(n, d)
    prev_g, nxt_g, acc_g = dev_t(prev, dev), dev_t(nxt, dev), dev_t(acc, dev)
    for kind, imm_r, imm_g in (("none", None, None), ("shared", imm[0], dev_t(imm[0], dev)),
                               ("per particle", imm, metrics.PerChainDiag(dev_t(imm, dev)))):
        m_g = pt.esjd(imm_g)(prev_g, nxt_g, acc_g)
        assert m_g.shape == (n,) and m_g.dtype == torch.float32 and m_g.is_cuda
        m, m_r = t2n(m_g), rp.esjd(prev, nxt, acc, imm_r)
        assert np.all(m[zero_rows] == 0) and np.all(np.isfinite(m)) and np.all(m >= 0), kind
        np.testing.assert_allclose(m, m_r, rtol=RTOL, atol=ATOL, err_msg=kind)
    tagged = metrics.PerChainDiagTensor.tag(dev_t(imm, dev))  # the form window_adaptation and the pretune hand on
    assert torch.equal(pt.esjd(tagged)(prev_g, nxt_g, acc_g), m_g)


def test_esjd_dense_metric(dev):
    """A shared dense (D, D) inverse mass matrix at D = 65: one Cholesky factor, one triangular solve, the kernel on
    the whitened difference; against acc * d^T imm^-1 d solved in fp64."""
    n, d = 257, 65
    prev, nxt, acc, zero_rows, _ = _esjd_inputs(n, d)
    rng = np.random.default_rng(65)
    a = rng.standard_normal((d, 4 * d))
    imm = (a @ a.T / (4 * d) + 0.5 * np.eye(d)).astype(f32)
    keep = np.setdiff1d(np.arange(n), zero_rows)
    m = t2n(pt.esjd(dev_t(imm, dev))(dev_t(prev, dev), dev_t(nxt, dev), dev_t(acc, dev)))
    ref = rp.esjd_dense64(prev[keep], nxt[keep], acc[keep], imm)
    err = np.abs(m[keep] - ref) / ref
    print("dense esjd, D = 65: largest relative error", err.max(), "condition number", np.linalg.cond(imm.astype(f64)))
    assert np.all(m[zero_rows] == 0)
    assert err.max() <= DENSE_RTOL


# ----------------------------------------------------------------------------- weights, ancestors
# one workgroup of 1024 threads that loops: one item, exactly one sweep, one more, two sweeps and one more
@pytest.mark.parametrize("alpha", [0.0, 0.1])
@pytest.mark.parametrize("n", [1, 1024, 1025, 2049])
def test_weights_and_ancestors_match_restatement(dev, n, alpha):
    rng = np.random.default_rng(n)
    measure = (rng.random(n) ** 3).astype(f32)
    measure[rng.random(n) < 0.2] = 0.0  # rejected trials
    for case, m in (("random", measure), ("all zero", np.zeros(n, f32))):
        w_g = pt.pretune_weights(dev_t(m, dev), alpha)
        w, w_r = t2n(w_g), rp.pretune_weights(m, alpha)
        assert w_g.shape == (n,) and w_g.dtype == torch.float32, case
        np.testing.assert_allclose(w, w_r, rtol=RTOL, atol=0, err_msg=case)
        assert abs(float(w.astype(f64).sum()) - 1.0) <= 1e-5
        if case == "all zero":  # uniform, through S == 0 (alpha 0) or through alpha / (N alpha)
            np.testing.assert_allclose(w, np.full(n, 1.0 / n), rtol=RTOL)
            if alpha == 0:
                assert np.array_equal(w, np.full(n, f32(1.0 / n), f32))
        # the ancestors the pretune draws, bit for bit those of the restatement GIVEN the device's own weights (a
        # last-place difference in a weight may legitimately move an ancestor)
        key = prng.key(7 * n + int(10 * alpha))
        a_g = smc.resampling.multinomial._bjx_trusted(key, w_g, n)
        assert np.array_equal(t2n(a_g), rx.multinomial(key, w, n)), case


# ----------------------------------------------------------------------------- jitter_gather
# K: the thread-per-row path, 4-byte sweeps, one 16-byte piece, a second (partial) 4-byte sweep; M < N and M > N
@pytest.mark.parametrize("log_space", [False, True])
@pytest.mark.parametrize("n,m", [(37, 53), (53, 37), (300, 1030)])
@pytest.mark.parametrize("k", [1, 3, 4, 65, 264])
def test_jitter_gather_is_bit_exact(dev, k, n, m, log_space):
    rng = np.random.default_rng(100 * k + n)
    p = rng.standard_normal((n, k)).astype(f32)
    anc = rng.integers(0, n, m).astype(np.int32)  # unsorted, repeated
    anc[:6] = [n - 1, 0, n - 1, 5, -3, n + 4]  # the last two are clamped to 0 and N - 1
    p_g, anc_g = dev_t(p, dev), dev_t(anc, dev)
    before = p_g.clone()
    key = prng.key(11 * k + m)
    sigmas = [f32(0.3), (0.05 + 0.5 * rng.random(k)).astype(f32)]
    for sigma in sigmas:
        sigma_g = float(sigma) if np.ndim(sigma) == 0 else dev_t(sigma, dev)
        out = pt.jitter_gather(key, p_g, anc_g, sigma_g, log_space)
        assert out.shape == (m, k) and out.data_ptr() != p_g.data_ptr()
        ref = rp.jitter_gather(key, p, anc, sigma, log_space)
        assert np.array_equal(bits(t2n(out)), bits(ref)), (k, n, m, log_space, np.ndim(sigma))
        if log_space:
            assert np.array_equal(np.signbit(t2n(out)), np.signbit(p[np.clip(anc, 0, n - 1)]))
    if k == 1:  # an (N,) vector is the K = 1 case and comes back as (M,)
        out = pt.jitter_gather(key, p_g[:, 0].contiguous(), anc_g, 0.3, log_space)
        assert out.shape == (m,) and np.array_equal(bits(t2n(out)), bits(rp.jitter_gather(key, p[:, 0], anc, f32(0.3),
                                                                                          log_space)))
    assert torch.equal(p_g, before)


# ----------------------------------------------------------------------------- pretune, full steps
def _case(inner, dev):
    ivp, ivl, x0, override, sigma = rp.step_case(inner)
    prior_g, lik_g = bjx.targets.DiagGaussian(dev_t(ivp, dev)), bjx.targets.DiagGaussian(dev_t(ivl, dev))
    override_g = {k: dev_t(v, dev) if isinstance(v, np.ndarray) else v for k, v in override.items()}
    sigma_g = {k: dev_t(v, dev) if np.ndim(v) else float(v) for k, v in sigma.items()}
    if inner == "mala":
        step_fn, init_fn = bjx.mala.build_kernel(), bjx.mala.init
    else:
        step_fn, init_fn = bjx.hmc.build_kernel(use_graph=False), bjx.hmc.init
    pretune_fn = pt.build_pretune(init_fn, step_fn, rp.CASE_ALPHA, sigma_g, rp.CASE_N,
                                  positive_parameters=rp.CASE_POSITIVE[inner])
    host = (otargets.diag_gaussian(ivp), otargets.diag_gaussian(ivl), x0, override, sigma)
    return host, (prior_g, lik_g, override_g, step_fn, init_fn, pretune_fn)


def _assert_override(new_g, new_r, override_g, sigma, leave_out):
    """Sampled entries at the position tolerance, rows in ``leave_out`` aside; every other entry the same object."""
    assert set(new_g) == set(new_r)
    assert leave_out.sum() <= 0.01 * len(leave_out)
    for name, value in new_g.items():
        if name in sigma:
            assert value.dtype == torch.float32 and value.is_cuda and value.shape == override_g[name].shape
            assert value.data_ptr() != override_g[name].data_ptr()
            np.testing.assert_allclose(t2n(value)[~leave_out], new_r[name][~leave_out], rtol=POS_TOL, atol=POS_TOL,
                                       err_msg=name)
        else:
            assert value is override_g[name]
    if "inverse_mass_matrix" in sigma:  # a sampled (N, D) matrix travels tagged as one diagonal per particle
        assert isinstance(new_g["inverse_mass_matrix"], metrics.PerChainDiagTensor)


@pytest.mark.parametrize("inner", ["mala", "hmc"])
def test_pretune_call_matches_restatement(dev, inner):
    """One ``pretune`` call at temperature 0.3 from identical inputs.  A position may be left out only where the
    restatement's own threshold lies within 2^-20 of a cumulative-weight boundary (none does at this key:
    test_smc_pretune_api.py)."""
    (prior, lik, x0, override, sigma), (prior_g, lik_g, override_g, step_fn, init_fn, pretune_fn) = _case(inner, dev)
    kernel = bjx.pretuning.build_kernel(bjx.tempered_smc, prior_g, lik_g, step_fn, init_fn,
                                        smc.resampling.systematic, pretune_fn, num_mcmc_steps=2)
    logdensity = kernel.tempered_logdensity
    logdensity.set_temperature(dev_t(rp.CASE_LMBDA, dev))
    inner_state = bjx.tempered_smc.init(dev_t(x0, dev))._replace(lmbda=dev_t(rp.CASE_LMBDA, dev))
    state = pt.StateWithParameterOverride(inner_state, override_g)
    snapshot = {k: v.clone() for k, v in override_g.items() if isinstance(v, torch.Tensor)}
    key = prng.key(rp.CASE_KEYS[inner][0])
    new_g = pretune_fn(key, state, logdensity)
    fn = rsmc.tempered_logdensity(prior, lik, rp.CASE_LMBDA)
    new_r, (_, acc, measure, weights, ancestors) = rp.pretune(key, x0, override, fn, rp.make_move(inner, rp.CASE_L),
                                                              rp.CASE_ALPHA, sigma, rp.CASE_POSITIVE[inner])
    assert np.count_nonzero(measure) > 0 and np.count_nonzero(acc < 1) > 0 and len(np.unique(ancestors)) < rp.CASE_N
    leave_out = rp.near_boundary(prng.split(key, 2)[1], weights)
    _assert_override(new_g, new_r, override_g, sigma, leave_out)
    for k, v in snapshot.items():  # the incoming override's tensors are untouched
        assert torch.equal(override_g[k], v)


def _resync(st_g):
    return rsmc.TemperedSMCState(t2n(st_g.particles), t2n(st_g.weights), f32(st_g.lmbda.item()))


def _assert_step(new_g, info_g, st_r, info_r):
    st_g, smc_info = new_g.sampler_state, info_g.smc_info
    assert isinstance(info_g, pt.SMCInfoWithParameterDistribution)
    assert info_g.parameter_override is new_g.parameter_override
    assert smc_info.ancestors.dtype == torch.int32 and np.array_equal(t2n(smc_info.ancestors), info_r.ancestors)
    assert np.array_equal(t2n(smc_info.update_info.is_accepted), info_r.update_info.is_accepted)
    np.testing.assert_allclose(t2n(st_g.particles), st_r.particles, rtol=POS_TOL, atol=POS_TOL)
    np.testing.assert_allclose(t2n(st_g.weights), st_r.weights, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(t2n(smc_info.log_likelihood_increment), info_r.log_likelihood_increment, rtol=RTOL,
                               atol=ATOL)
    assert st_g.lmbda.shape == () and st_g.lmbda.is_cuda


@pytest.mark.parametrize("inner", ["mala", "hmc"])
def test_pretuning_steps_match_restatement(dev, inner):
    """One full step of ``pretuning`` around ``tempered_smc`` (``lmbda=``) and one around ``adaptive_tempered_smc``,
    each from the initial state: the new override at the position tolerance, then the SMC step made with it --
    ancestors and accept bits exact, particles at the position tolerance, weights and the increment at the standing
    tolerances."""
    (prior, lik, x0, override, sigma), (prior_g, lik_g, override_g, step_fn, init_fn, pretune_fn) = _case(inner, dev)
    move_of, positive = rp.make_move(inner, rp.CASE_L), rp.CASE_POSITIVE[inner]
    _, k_fixed, k_adaptive = (prng.key(s) for s in rp.CASE_KEYS[inner])
    common = (prior_g, lik_g, step_fn, init_fn, smc.resampling.systematic, override_g, pretune_fn)

    def leave_out(key):
        fn = rsmc.tempered_logdensity(prior, lik, f32(0.0))
        pretune_key = prng.split(key, 2)[1]
        _, details = rp.pretune(pretune_key, x0, override, fn, move_of, rp.CASE_ALPHA, sigma, positive)
        return rp.near_boundary(prng.split(pretune_key, 2)[1], details[3])

    fixed = bjx.pretuning(bjx.tempered_smc, *common, num_mcmc_steps=2)
    st_g = fixed.init(dev_t(x0, dev))
    assert st_g.parameter_override is override_g and float(st_g.sampler_state.lmbda) == 0.0
    new_g, info_g = fixed.step(k_fixed, st_g, lmbda=0.4)
    st_r, new_r, info_r = rp.pretuned_step(k_fixed, rsmc.init(x0), override, f32(0.4), prior, lik, move_of, 2,
                                           rp.CASE_ALPHA, sigma, positive)
    _assert_override(new_g.parameter_override, new_r, override_g, sigma, leave_out(k_fixed))
    _assert_step(new_g, info_g, st_r, info_r)
    assert f32(new_g.sampler_state.lmbda.item()) == f32(0.4)
    assert 0 < int(info_r.update_info.is_accepted.sum())

    adaptive = bjx.pretuning(bjx.adaptive_tempered_smc, *common, num_mcmc_steps=2, target_ess=0.5)
    st_g = adaptive.init(dev_t(x0, dev))
    new_g, info_g = adaptive.step(k_adaptive, st_g)
    lam_g = f32(new_g.sampler_state.lmbda.item())
    _, lam_r = rsmc.next_temperature(lik(x0)[0], 0.5, f32(0.0))
    assert abs(float(lam_g) - float(lam_r)) <= DELTA_TOL and 0 < lam_g < 1
    # the rest of the step at the temperature the device chose
    st_r, new_r, info_r = rp.pretuned_step(k_adaptive, rsmc.init(x0), override, lam_g, prior, lik, move_of, 2,
                                           rp.CASE_ALPHA, sigma, positive)
    _assert_override(new_g.parameter_override, new_r, override_g, sigma, leave_out(k_adaptive))
    _assert_step(new_g, info_g, st_r, info_r)


# ----------------------------------------------------------------------------- shared entries, no host read
def test_shared_entries_pass_through_and_a_step_reads_nothing_back(dev):
    """Only ``step_size`` is sampled: the shared ``(D,)`` inverse mass matrix (which is also the ESJD's metric) and the
    trajectory length come back as the same objects, step after step.  After a first step (which compiles and caches
    what it needs) a step of either algorithm under ``torch.cuda.set_sync_debug_mode("error")`` raises nothing."""
    n, d = 64, 3
    ivp, ivl, x0, _, _ = rp.step_case("hmc")
    prior_g, lik_g = bjx.targets.DiagGaussian(dev_t(ivp, dev)), bjx.targets.DiagGaussian(dev_t(ivl, dev))
    imm = dev_t(np.linspace(0.5, 1.5, d).astype(f32), dev)
    override = {"step_size": torch.full((n,), 0.3, device=dev), "inverse_mass_matrix": imm, "num_integration_steps": 2}
    step_fn, init_fn = bjx.hmc.build_kernel(use_graph=False), bjx.hmc.init
    pretune_fn = pt.build_pretune(init_fn, step_fn, 0.05, {"step_size": 0.1}, n, positive_parameters=("step_size",))
    common = (prior_g, lik_g, step_fn, init_fn, smc.resampling.systematic, override, pretune_fn)
    fixed = bjx.pretuning(bjx.tempered_smc, *common, num_mcmc_steps=1)
    adaptive = bjx.pretuning(bjx.adaptive_tempered_smc, *common, num_mcmc_steps=1, target_ess=0.5)
    keys = prng.split(prng.key(9), 4)
    st_f, _ = fixed.step(keys[0], fixed.init(dev_t(x0, dev)), lmbda=0.1)
    st_a, _ = adaptive.step(keys[1], adaptive.init(dev_t(x0, dev)))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        st_f, info_f = fixed.step(keys[2], st_f, lmbda=0.3)
        st_a, info_a = adaptive.step(keys[3], st_a)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for st, info in ((st_f, info_f), (st_a, info_a)):
        new = st.parameter_override
        assert new["inverse_mass_matrix"] is imm and new["num_integration_steps"] is override["num_integration_steps"]
        assert info.parameter_override is new and new["step_size"] is not override["step_size"]
        step = t2n(new["step_size"])
        assert step.shape == (n,) and np.all(step > 0) and len(np.unique(step)) > 1
        assert bool(torch.isfinite(st.sampler_state.weights).all())
    assert torch.equal(override["step_size"], torch.full((n,), 0.3, device=dev))
