"""GPU parity of multinomial / residual resampling, the waste-free row store, waste-free tempered SMC, the particle
moments and inner-kernel tuning (blackjax_amd/smc/, csrc/bjx_smc.hip, include/bjx_hip.h "SMC") against the NumPy
restatement, tests/smc_extra_restatement.py."""
import numpy as np
import pytest
import torch

import blackjax_amd as bjx
import random_walk_restatement as rrw
import smc_extra_restatement as rx
import smc_restatement as rsmc
from blackjax_amd import random_walk as prw
from blackjax_amd import smc
from blackjax_amd.smc.tuning import from_particles
from oracle import prng, targets as otargets

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64

RTOL, ATOL = 1e-6, 1e-7  # tests/test_smc_gpu.py: fp64-summed scalars rounded to fp32
DELTA_TOL = 1e-4  # tests/test_smc_gpu.py: the temperature against the interval searched


def t2n(t):
    return t.detach().cpu().numpy()


def dev_t(a, dev):
    return torch.as_tensor(np.asarray(a), device=dev)


# ----------------------------------------------------------------------------- resampling
def _weight_sets(n, m):
    rng = np.random.default_rng(1000 * n + m)
    sets = {"uniform": np.full(n, f32(1.0 / n), f32)}
    g = rng.gamma(0.5, size=n)
    if n > 1:
        g[::5] = 0.0
        g[-1] = max(g[-1], 0.1)
    sets["gamma"] = (g / g.sum()).astype(f32)
    one = np.zeros(n, f32)
    one[n // 2] = 1.0
    sets["one"] = one
    # w_j = k_j / M: exactly so when M is a power of two (then S == M and nothing is drawn)
    k = np.bincount(rng.integers(0, n, m), minlength=n)
    sets["counts"] = (k / f64(m)).astype(f32)
    if 4 * m < 3 * n:  # every w_j < 1 / M: S == 0, every position is drawn
        r = 0.75 + 0.25 * rng.random(n)
        sets["below"] = (r / r.sum()).astype(f32)
    return sets


@pytest.mark.parametrize("n,m", [(1, 1), (7, 7), (1024, 1024), (1025, 1023), (1025, 1025), (2049, 512), (512, 2049)])
def test_multinomial_and_residual_match_restatement(dev, n, m):
    """Ancestors bit for bit on both sides of the 1024-item scan tile, for the weights and for the M + 1 exponentials."""
    for kind, w in _weight_sets(n, m).items():
        w_g = dev_t(w, dev)
        key = prng.key(7 * n + m)
        cnt, _ = rx.residual_split(w, m)
        if kind == "counts" and m & (m - 1) == 0:
            assert cnt.sum() == m
        if kind == "below" or (kind == "uniform" and n > m):
            assert cnt.sum() == 0
        for name in ("multinomial", "residual"):
            a_g = getattr(smc.resampling, name)(key, w_g, m)
            a_r = getattr(rx, name)(key, w, m)
            assert a_g.dtype == torch.int32 and a_g.shape == (m,) and a_g.is_cuda
            a = t2n(a_g)
            assert a.min() >= 0 and a.max() < n
            assert np.array_equal(a, a_r), (name, kind, n, m, int((a != a_r).sum()))
            assert np.array_equal(t2n(getattr(smc.resampling, name)._bjx_trusted(key, w_g, m)), a_r)
            if name == "multinomial":
                assert np.all(np.diff(a) >= 0)
            else:
                assert np.all(np.bincount(a, minlength=n) >= cnt)


def test_resampling_validation(dev):
    n = 16
    w = torch.full((n,), 1.0 / n, device=dev)
    key = prng.key(1)
    for fn in (smc.resampling.multinomial, smc.resampling.residual):
        with pytest.raises(RuntimeError):
            fn(key, torch.full((n,), 1.0 / n), n)  # host tensor: there is no CPU fallback
        with pytest.raises(ValueError):
            fn(key, w.reshape(4, 4), n)
        with pytest.raises(ValueError):
            fn(key, 2.0 * w, n)  # not normalised
        with pytest.raises(ValueError):
            fn(key, w, (1 << 24) + 1)
        with pytest.raises(ValueError):
            fn(key, torch.zeros(0, device=dev), 4)
        assert fn(key, w, 0).shape == (0,)


# ----------------------------------------------------------------------------- the strided row store
@pytest.mark.parametrize("d", [1, 3, 4, 65])
@pytest.mark.parametrize("m,p", [(1, 2), (5, 3), (257, 4)])
def test_scatter_rows_matches_slicing(dev, d, m, p):
    rng = np.random.default_rng(100 * d + m)
    out = rng.standard_normal((m * p, d)).astype(f32)
    out_g = dev_t(out, dev)
    x0 = rng.standard_normal((m, d)).astype(f32)
    smc.waste_free.scatter_rows(dev_t(x0, dev), 0, 1, out_g)
    out[:m] = x0
    assert np.array_equal(t2n(out_g).view(np.int32), out.view(np.int32))
    for t in range(p - 1):  # each call owns rows M + t + i (p - 1); every other row keeps its bytes
        x = rng.standard_normal((m, d)).astype(f32)
        x_g = dev_t(x, dev)
        smc.waste_free.scatter_rows(x_g, m + t, p - 1, out_g)
        out[m + t::p - 1] = x
        assert np.array_equal(t2n(out_g).view(np.int32), out.view(np.int32))
        assert np.array_equal(t2n(x_g).view(np.int32), x.view(np.int32))
    with pytest.raises(ValueError):
        smc.waste_free.scatter_rows(dev_t(x0, dev), m + p - 1, p - 1, out_g)  # the last row would be row M p


def test_scatter_rows_takes_the_4_byte_path_for_an_unaligned_array(dev):
    m, d, p = 9, 4, 3
    rng = np.random.default_rng(0)
    flat = rng.standard_normal(m * p * d + 1).astype(f32)
    flat_g = dev_t(flat, dev)
    out_g = flat_g[1:].view(m * p, d)  # 4 bytes past a 16-byte boundary
    x = rng.standard_normal((m, d)).astype(f32)
    smc.waste_free.scatter_rows(dev_t(x, dev), m + 1, p - 1, out_g)
    expect = flat.copy()
    expect[1:].reshape(m * p, d)[m + 1::p - 1] = x
    assert np.array_equal(t2n(flat_g).view(np.int32), expect.view(np.int32))


# ----------------------------------------------------------------------------- waste-free tempered SMC
WF_N = 256


def _step_case(d):
    """tests/test_smc_gpu.py's case: zero-mean diagonal Gaussians as prior and likelihood."""
    ivp = np.linspace(0.5, 2.0, d).astype(f32)
    ivl = (np.linspace(1.0, 3.0, d) * (3.5 / np.sqrt(d))).astype(f32)
    x0 = (prng.normal(prng.key(3), (WF_N, d)) / np.sqrt(ivp)).astype(f32)
    return ivp, ivl, x0


def _inner(name, d):
    if name == "mala":
        tau = f32(0.4 * d ** (-1.0 / 3.0))
        return bjx.mala.build_kernel(), bjx.mala.init, {"step_size": float(tau)}, rsmc.mala_move(tau)
    step = rrw.normal(0.5)
    move = rsmc.Move(rrw.init, lambda keys, st, fn: rrw.additive_step_kernel(None, st, fn, step,
                                                                             chain_keys_override=keys))
    return (bjx.additive_step_random_walk.build_kernel(), bjx.additive_step_random_walk.init,
            {"random_step": prw.normal(0.5)}, move)


def _resync(st_g):
    return rsmc.TemperedSMCState(t2n(st_g.particles), t2n(st_g.weights), f32(st_g.lmbda.item()))


def _assert_wf_step(st_g, info_g, st_r, info_r, x_before, p):
    m = WF_N // p
    assert info_g.ancestors.dtype == torch.int32 and info_g.ancestors.shape == (m,)
    assert np.array_equal(t2n(info_g.ancestors), info_r.ancestors)
    assert isinstance(info_g.update_info, tuple) and len(info_g.update_info) == p - 1
    for i_g, i_r in zip(info_g.update_info, info_r.update_info):
        assert i_g.is_accepted.shape == (m,) and np.array_equal(t2n(i_g.is_accepted), i_r.is_accepted)
    assert st_g.particles.shape == (WF_N, x_before.shape[1])
    np.testing.assert_allclose(t2n(st_g.particles), st_r.particles, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(t2n(st_g.weights), st_r.weights, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(t2n(info_g.log_likelihood_increment), info_r.log_likelihood_increment, rtol=RTOL,
                               atol=ATOL)
    # the layout: rows [0, M) are the resampled particles, bit for bit
    assert torch.equal(st_g.particles[:m], smc.base.gather(x_before, info_g.ancestors))


@pytest.mark.parametrize("d", [3, 8])
@pytest.mark.parametrize("p", [2, 4])
@pytest.mark.parametrize("inner", ["mala", "normal_random_walk"])
def test_waste_free_steps_match_restatement(dev, d, p, inner):
    """One step of a fixed schedule and a three-step run, then the adaptive sampler, every step checked from the
    GPU's own previous state."""
    ivp, ivl, x0 = _step_case(d)
    prior_r, lik_r = otargets.diag_gaussian(ivp), otargets.diag_gaussian(ivl)
    prior_g, lik_g = bjx.targets.DiagGaussian(dev_t(ivp, dev)), bjx.targets.DiagGaussian(dev_t(ivl, dev))
    step_fn, init_fn, params, move = _inner(inner, d)
    strategy = smc.waste_free_smc(WF_N, p)

    fixed = bjx.tempered_smc(prior_g, lik_g, step_fn, init_fn, params, smc.resampling.systematic,
                             num_mcmc_steps=None, update_strategy=strategy)
    st_g = fixed.init(dev_t(x0, dev))
    for k, lam in zip(prng.split(prng.key(11), 3), (0.1, 0.4, 1.0)):
        st_prev, x_before = _resync(st_g), st_g.particles
        st_g, info_g = fixed.step(k, st_g, lam)
        st_r, info_r = rx.tempered_step(k, st_prev, f32(lam), prior_r, lik_r, move, None, rsmc.systematic, p)
        _assert_wf_step(st_g, info_g, st_r, info_r, x_before, p)
        assert f32(st_g.lmbda.item()) == f32(lam)

    adaptive = bjx.adaptive_tempered_smc(prior_g, lik_g, step_fn, init_fn, params, smc.resampling.stratified, 0.5,
                                         num_mcmc_steps=None, update_strategy=strategy)
    st_g = adaptive.init(dev_t(x0, dev))
    lams = []
    for k in prng.split(prng.key(12), 3):
        st_prev, x_before = _resync(st_g), st_g.particles
        st_g, info_g = adaptive.step(k, st_g)
        lam_g = f32(st_g.lmbda.item())
        _, lam_r = rsmc.next_temperature(lik_r(st_prev.particles)[0], 0.5, st_prev.lmbda)  # all N particles
        assert abs(float(lam_g) - float(lam_r)) <= DELTA_TOL * (1.0 - float(st_prev.lmbda))
        st_r, info_r = rx.tempered_step(k, st_prev, lam_g, prior_r, lik_r, move, None, rsmc.stratified, p)
        _assert_wf_step(st_g, info_g, st_r, info_r, x_before, p)
        lams.append(float(lam_g))
        if lam_g == 1:
            break
    assert all(b > a for a, b in zip([0.0] + lams, lams)) and lams[-1] <= 1.0


def test_waste_free_validation(dev):
    d = 4
    prior = bjx.targets.DiagGaussian(torch.ones(d, device=dev))
    alg = bjx.tempered_smc(prior, prior, bjx.mala.build_kernel(), bjx.mala.init, {"step_size": 0.1},
                           smc.resampling.systematic, num_mcmc_steps=3, update_strategy=smc.waste_free_smc(16, 4))
    st = alg.init(torch.zeros(16, d, device=dev))
    with pytest.raises(ValueError):
        alg.step(prng.key(1), st, 0.5)  # waste-free sets its own number of transitions
    alg = bjx.tempered_smc(prior, prior, bjx.mala.build_kernel(), bjx.mala.init, {"step_size": 0.1},
                           smc.resampling.systematic, num_mcmc_steps=None, update_strategy=smc.waste_free_smc(32, 4))
    with pytest.raises(ValueError):
        alg.step(prng.key(1), st, 0.5)  # built for another number of particles


# ----------------------------------------------------------------------------- moments
@pytest.mark.parametrize("n", [1, 2, 255, 257, 1023, 1025, 4097])  # the row tile is 256: one tile, two, ragged, 17
@pytest.mark.parametrize("d", [1, 3, 64, 257])
def test_particle_moments_match_fp64(dev, n, d):
    rng = np.random.default_rng(10 * n + d)
    x = (rng.standard_normal((n, d)) * rng.uniform(0.1, 5.0, d) + rng.uniform(-20.0, 20.0, d)).astype(f32)
    x_g = dev_t(x, dev)
    atol = 1e-7 * float(np.abs(x).max())
    mean_g, std_g = from_particles.particles_means(x_g), from_particles.particles_stds(x_g)
    assert mean_g.shape == (d,) and std_g.shape == (d,) and mean_g.dtype == std_g.dtype == torch.float32
    np.testing.assert_allclose(t2n(mean_g), x.astype(f64).mean(0), rtol=1e-6, atol=atol)
    np.testing.assert_allclose(t2n(std_g), x.astype(f64).std(0), rtol=1e-6, atol=atol)
    np.testing.assert_allclose(t2n(mean_g), rx.particles_means(x), rtol=1e-6, atol=atol)
    np.testing.assert_allclose(t2n(std_g), rx.particles_stds(x), rtol=1e-6, atol=atol)
    if n == 1:
        assert np.all(t2n(std_g) == 0)
    # reproducible: a second evaluation, with another workspace, gives the same bits
    assert torch.equal(from_particles.particles_stds(x_g), std_g)
    assert from_particles.particles_as_rows(x_g) is x_g
    ok = t2n(std_g) > 0
    np.testing.assert_allclose(t2n(from_particles.mass_matrix_from_particles(x_g))[ok],
                               1.0 / x.astype(f64).var(0)[ok], rtol=1e-5)


@pytest.mark.parametrize("n,d", [(2, 3), (1025, 8), (4097, 65)])
def test_particle_covariance(dev, n, d):
    """Per entry within 2 N 2^-24 sum_k |c_ki c_kj| / (N - 1): the fp32 dot-product bound, doubled for the fp32
    rounding of the centred rows; c the fp64 centred rows."""
    rng = np.random.default_rng(n + d)
    x = (rng.standard_normal((n, d)) @ rng.standard_normal((d, d)) + rng.uniform(-5.0, 5.0, d)).astype(f32)
    cov_g = t2n(from_particles.particles_covariance_matrix(dev_t(x, dev))).astype(f64)
    c = x.astype(f64) - x.astype(f64).mean(0)
    bound = 2.0 * n * 2.0 ** -24 * (np.abs(c).T @ np.abs(c)) / (n - 1)
    err = np.abs(cov_g - rx.particles_covariance_matrix(x))
    print("largest error / bound", (err / bound).max())
    assert cov_g.shape == (d, d) and np.all(err <= bound)


# ----------------------------------------------------------------------------- inner-kernel tuning
IKT_N, IKT_D, IKT_L = 512, 4, 3


def _ikt_case(dev):
    ivp, ivl, _ = _step_case(IKT_D)
    x0 = (prng.normal(prng.key(4), (IKT_N, IKT_D)) / np.sqrt(ivp)).astype(f32)
    eps = f32(0.6 * IKT_D ** (-0.25))
    return ivp, ivl, x0, eps


def _update_g(eps, n_leapfrog=IKT_L):
    def update(rng_key, state, info):
        stds = from_particles.particles_stds(state.particles)
        return {"step_size": float(eps), "inverse_mass_matrix": stds * stds, "num_integration_steps": n_leapfrog}

    return update


def test_inner_kernel_tuning_matches_restatement(dev, monkeypatch):
    """tempered_smc with hmc whose inverse mass matrix is re-estimated each step as particles_stds(particles)**2:
    three steps, ancestors and accept bits exact, particles to tolerance; a step reads nothing back."""
    ivp, ivl, x0, eps = _ikt_case(dev)
    prior_r, lik_r = otargets.diag_gaussian(ivp), otargets.diag_gaussian(ivl)
    prior_g, lik_g = bjx.targets.DiagGaussian(dev_t(ivp, dev)), bjx.targets.DiagGaussian(dev_t(ivl, dev))
    imm0 = np.ones(IKT_D, f32)
    alg = bjx.inner_kernel_tuning(bjx.tempered_smc, prior_g, lik_g, bjx.hmc.build_kernel(), bjx.hmc.init,
                                  smc.resampling.systematic, _update_g(eps),
                                  {"step_size": float(eps), "inverse_mass_matrix": dev_t(imm0, dev),
                                   "num_integration_steps": IKT_L}, num_mcmc_steps=2)
    st_g = alg.init(dev_t(x0, dev))
    assert isinstance(st_g, smc.inner_kernel_tuning.StateWithParameterOverride)
    assert float(st_g.sampler_state.lmbda) == 0.0

    def make_move(imm):
        return rsmc.hmc_move(eps, imm, IKT_L)

    def update_r(rng_key, state, info):
        s = rx.particles_stds(state.particles)
        return (s * s).astype(f32)

    def forbidden(*args, **kwargs):
        raise AssertionError("a step read a value back to the host")

    imm_r, moved = imm0, False
    for k, lam in zip(prng.split(prng.key(21), 3), (0.1, 0.4, 1.0)):
        st_prev = _resync(st_g.sampler_state)
        imm_prev = t2n(st_g.parameter_override["inverse_mass_matrix"])
        np.testing.assert_allclose(imm_prev, imm_r, rtol=2e-6)
        with monkeypatch.context() as mp:
            for name in ("item", "tolist", "cpu", "numpy", "__bool__", "__float__", "__int__"):
                mp.setattr(torch.Tensor, name, forbidden)
            st_g, info_g = alg.step(k, st_g, lmbda=lam)
        # the restatement moves with the GPU's own mass matrix (one ulp of it would legitimately move a trajectory)
        st_r, imm_r, info_r = rx.inner_kernel_tuning_step(k, st_prev, imm_prev, f32(lam), prior_r, lik_r, make_move,
                                                          update_r, 2)
        inner = st_g.sampler_state
        assert np.array_equal(t2n(info_g.ancestors), info_r.ancestors)
        assert np.array_equal(t2n(info_g.update_info.is_accepted), info_r.update_info.is_accepted)
        np.testing.assert_allclose(t2n(inner.particles), st_r.particles, rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(t2n(inner.weights), st_r.weights, rtol=RTOL, atol=ATOL)
        assert f32(inner.lmbda.item()) == f32(lam)
        moved = moved or bool(np.any(np.abs(imm_r - 1.0) > 0.05))
    np.testing.assert_allclose(t2n(st_g.parameter_override["inverse_mass_matrix"]), imm_r, rtol=2e-6)
    assert moved  # the override did change


def _counted(fn):
    calls = [0]

    def wrapped(q):
        calls[0] += 1
        return fn(q)

    return wrapped, calls


def test_inner_kernel_tuning_builds_once(dev):
    """After three steps ``kernel.tempered_logdensity`` is the object it was, and the user's log-prior has been called
    by Python no more often than after the FIRST step of an untuned tempered_smc with the same callables.  One HMC
    transition of one leapfrog step per temperature: the three steps stay below the 16th evaluation, at which
    ``value_and_grad`` re-checks a generated kernel against the Python function whoever drives it."""
    n_mcmc, n_leapfrog = 1, 1

    def logprior(q):
        return -0.5 * (q * q).sum(-1)

    def loglik(q):
        return -2.0 * ((q - 1.5) ** 2).sum(-1)

    x0 = dev_t(prng.normal(prng.key(5), (IKT_N, IKT_D)), dev)
    params = {"step_size": 0.3, "inverse_mass_matrix": torch.ones(IKT_D, device=dev),
              "num_integration_steps": n_leapfrog}
    (prior_u, calls_u), (lik_u, _) = _counted(logprior), _counted(loglik)
    untuned = bjx.tempered_smc(prior_u, lik_u, bjx.hmc.build_kernel(), bjx.hmc.init, params,
                               smc.resampling.systematic, num_mcmc_steps=n_mcmc)
    untuned.step(prng.key(1), untuned.init(x0), 0.2)

    (prior_t, calls_t), (lik_t, lik_calls_t) = _counted(logprior), _counted(loglik)
    kernel = bjx.inner_kernel_tuning.build_kernel(bjx.tempered_smc, prior_t, lik_t, bjx.hmc.build_kernel(),
                                                  bjx.hmc.init, smc.resampling.systematic,
                                                  _update_g(0.3, n_leapfrog), num_mcmc_steps=n_mcmc)
    logdensity = kernel.tempered_logdensity
    state = smc.inner_kernel_tuning.init(bjx.tempered_smc.init, x0, params)
    after_first = None
    for k, lam in zip(prng.split(prng.key(2), 3), (0.2, 0.6, 1.0)):
        state, _ = kernel(k, state, lmbda=lam)
        assert kernel.tempered_logdensity is logdensity
        if after_first is None:
            after_first = (calls_t[0], lik_calls_t[0])
    print("python calls of the log-prior: tuned, 3 steps", calls_t[0], "untuned, 1 step", calls_u[0])
    assert calls_t[0] <= calls_u[0] and (calls_t[0], lik_calls_t[0]) == after_first
    assert bool(torch.isfinite(state.sampler_state.weights).all())
