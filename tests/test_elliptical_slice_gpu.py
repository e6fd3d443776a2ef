"""GPU parity of the elliptical slice sampler (blackjax_amd/elliptical_slice.py, csrc/bjx_ess.hip, include/bjx_hip.h
"elliptical slice") against the NumPy restatement of the reference's arithmetic,
tests/elliptical_slice_restatement.py."""
import importlib

import numpy as np
import pytest
import torch

import blackjax_amd as bjx
import elliptical_slice_restatement as ress
from elliptical_slice_restatement import COV, MEAN, OBS, PREC, moment_errors, posterior_draws
from oracle import prng, targets as otargets

pytestmark = pytest.mark.gpu
pess = importlib.import_module("blackjax_amd.elliptical_slice")  # (the package attribute is the API object)
f32 = np.float32


def t2n(t):
    return t.detach().cpu().numpy()


def dev_t(a, dev):
    return torch.as_tensor(np.asarray(a), device=dev)


def same_bits(a, b):
    if a.dtype == torch.float32:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def _gaussian_case(N, D):
    """Likelihood, start and prior of the parity cases: sigma_j = 10^(-0.5 + j / (D - 1)) and q0 = normal(key(1)) * sigma
    as in test_mala_gpu._gaussian_case; prior mean 0.5 (-1)^j, prior variances sigma_j^2."""
    sig = (10.0 ** (-0.5 + 1.0 * np.arange(D) / max(D - 1, 1))).astype(f32)
    inv_var = (f32(1) / (sig * sig)).astype(f32)
    q0 = (prng.normal(prng.key(1), (N, D)) * sig).astype(f32)
    mean = (0.5 * (-1.0) ** np.arange(D)).astype(f32)
    return inv_var, q0, mean, (sig * sig).astype(f32)


def _assert_transition(st_g, info_g, st_r, info_r):
    assert info_g.subiter.dtype == torch.int32 and info_g.theta.dtype == torch.float32
    assert np.array_equal(t2n(info_g.subiter), info_r.subiter)
    assert np.array_equal(t2n(info_g.theta).view(np.int32), info_r.theta.view(np.int32))
    np.testing.assert_allclose(t2n(st_g.position), st_r.position, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(t2n(info_g.momentum), info_r.momentum, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(t2n(st_g.logdensity), st_r.logdensity, rtol=1e-6, atol=1e-6)


def _run_parity(dev, N, D, cov, n_steps, chol_t=None):
    inv_var, q0, mean, _ = _gaussian_case(N, D)
    fn_r = otargets.diag_gaussian(inv_var)
    alg = bjx.elliptical_slice(bjx.targets.DiagGaussian(dev_t(inv_var, dev)), mean=dev_t(mean, dev),
                               cov=dev_t(cov, dev), chain_offset=3)
    st_g = alg.init(dev_t(q0, dev))
    st_r = ress.init(q0, fn_r)
    np.testing.assert_allclose(t2n(st_g.logdensity), st_r.logdensity, rtol=1e-6, atol=1e-6)
    counts = []
    for k in prng.split(prng.key(9), n_steps):
        st_r, info_r = ress.kernel(k, st_r, fn_r, mean=mean, cov=cov, chain_offset=3, chol_t=chol_t)
        st_g, info_g = alg.step(k, st_g)
        _assert_transition(st_g, info_g, st_r, info_r)
        counts.append(info_r.subiter)
    counts = np.concatenate(counts)
    print(f"N={N} D={D}: subiter mean {counts.mean():.2f} max {counts.max()} ones {(counts == 1).sum()}")
    assert np.any(counts == 1) and np.any(counts >= 3)  # first-proposal accepts and repeated shrinking both occur


# (N, D): 4-byte sweep; one element; one 16-byte span; 4-byte sweep past 256 floats; 16-byte multi-span, full and ragged
@pytest.mark.parametrize("N,D", [(37, 10), (5, 1), (16, 64), (33, 260), (6, 1032), (3, 2052)])
def test_ess_diag_transitions_match_restatement(dev, N, D):
    """init + 5 consecutive transitions without re-sync, chain_offset = 3, diagonal prior: sub-iteration counts exact,
    theta bit-equal, positions / momenta / log-likelihoods within 1e-6 (the tolerances of test_mala_gpu.py)."""
    _run_parity(dev, N, D, _gaussian_case(N, D)[3], 5)


@pytest.mark.parametrize("N,D", [(24, 20), (130, 128)])
def test_ess_dense_transitions_match_restatement(dev, N, D):
    """The same over 3 transitions with the dense AR(1) prior covariance: nu = n @ L^T on the MFMA GEMM, restated as
    the fp32 fma chain in the engine's k order.  Both sides use the engine's fp32 factor, checked against NumPy's own
    to 1 ulp (two fp64 LAPACK builds may round a few of its entries differently, as in test_dense_gpu.py)."""
    cov = otargets.ar1_covariance(0.7, D)
    chol_t = t2n(pess._prepare_prior(0.0, dev_t(cov, dev), D, dev).chol_t)
    np.testing.assert_allclose(chol_t, ress.cholesky_t(cov), rtol=2.5e-7, atol=1e-9)
    _run_parity(dev, N, D, cov, 3, chol_t=chol_t)


def test_ess_is_shard_invariant_and_chain_major(dev):
    """Chains are keyed by their GLOBAL index: chains [0, 10) and [10, 24) run with chain_offset 3 and 13 reproduce
    the unsplit run bit for bit.  A chain-major key through run_inference_algorithm equals the restatement driven
    with chain i's keys split(split(key, .)[3 + i], .)[t]; the stacked history keeps subiter as int32 (T, N)."""
    N, D = 24, 64
    inv_var, q0, mean, cov = _gaussian_case(N, D)
    fn = bjx.targets.DiagGaussian(dev_t(inv_var, dev))
    q0_g = dev_t(q0, dev)

    def run(lo, hi):
        alg = bjx.elliptical_slice(fn, mean=dev_t(mean, dev), cov=dev_t(cov, dev), chain_offset=3 + lo)
        st = alg.init(q0_g[lo:hi].contiguous())
        for k in prng.split(prng.key(9), 4):
            st, info = alg.step(k, st)
        return st, info

    full, info_full = run(0, N)
    a, info_a = run(0, 10)
    b, info_b = run(10, N)
    for f, x, y in zip(full, a, b):
        assert same_bits(f, torch.cat([x, y]))
    for f, x, y in zip(info_full, info_a, info_b):
        assert same_bits(f, torch.cat([x, y]))

    T = 4
    alg = bjx.elliptical_slice(fn, mean=dev_t(mean, dev), cov=dev_t(cov, dev), chain_offset=3)
    st_g, (hist_state, hist_info) = bjx.util.run_inference_algorithm(prng.key(21), alg, T, initial_state=alg.init(q0_g),
                                                                     key_layout="chain_major")
    assert hist_info.subiter.dtype == torch.int32 and hist_info.subiter.shape == (T, N)
    assert hist_state.position.shape == (T, N, D) and hist_info.momentum.shape == (T, N, D)
    fn_r = otargets.diag_gaussian(inv_var)
    st_r = ress.init(q0, fn_r)
    chain_keys = prng.split(prng.key(21), N, offset=3)
    for t in range(T):
        st_r, info_r = ress.kernel(None, st_r, fn_r, mean=mean, cov=cov,
                                   chain_keys_override=prng.split(chain_keys, 1, offset=t)[:, 0])
        assert np.array_equal(t2n(hist_info.subiter[t]), info_r.subiter)
        assert np.array_equal(t2n(hist_info.theta[t]).view(np.int32), info_r.theta.view(np.int32))
        np.testing.assert_allclose(t2n(hist_state.position[t]), st_r.position, rtol=1e-6, atol=1e-6)
    # and the chain-major transitions differ from the step-major ones of the same key
    st_s, _ = alg.step(prng.key(21), alg.init(q0_g))
    assert not torch.equal(st_s.position, hist_state.position[0])


def test_ess_plain_pytorch_likelihood_with_a_hard_constraint(dev):
    """A value-only PyTorch callable with a hard constraint (-inf outside q_0 > 0): it is called on tensors that do not
    require grad, every chain stays inside the constraint, and the state's logdensity is the callable at its position
    bit for bit.  No parity claim: torch's fp32 row sum is not the restatement's."""
    N, D = 256, 8
    ninf = torch.tensor(float("-inf"), device=dev)

    def loglik(q):
        assert not q.requires_grad and not torch.is_grad_enabled()
        return torch.where(q[:, 0] > 0, -0.5 * (q * q).sum(-1), ninf)

    q0 = dev_t(prng.normal(prng.key(3), (N, D)), dev)
    q0[:, 0] = q0[:, 0].abs() + 0.1
    alg = bjx.elliptical_slice(loglik, mean=0.0, cov=torch.ones(D))
    st = alg.init(q0)
    n_shrunk = 0
    for k in prng.split(prng.key(5), 10):
        st, info = alg.step(k, st)
        assert bool((st.position[:, 0] > 0).all()) and bool(torch.isfinite(st.logdensity).all())
        with torch.no_grad():
            assert same_bits(st.logdensity, loglik(st.position))
        assert bool((info.subiter >= 1).all())
        n_shrunk += int((info.subiter > 1).sum())
    assert n_shrunk > 0


def test_ess_is_stationary_on_the_device_and_out_of_place(dev):
    """The conjugate case of test_elliptical_slice_api.py on the device, its likelihood a plain PyTorch callable: 4 096
    chains started in the posterior are still distributed as it after 30 transitions (means and variances within 5
    standard errors; the prior mean is not 0, so a mean entered in the wrong place fails).  ``step`` leaves the
    tensors of the state it was given untouched."""
    N, T = 4096, 30
    obs, prec = dev_t(OBS, dev), dev_t(PREC, dev)

    def loglik(q):
        d = q.double() - obs
        return (-0.5 * (prec * d * d).sum(-1)).float()

    alg = bjx.elliptical_slice(loglik, mean=dev_t(MEAN.astype(f32), dev), cov=dev_t(COV.astype(f32), dev))
    st = alg.init(dev_t(posterior_draws(N), dev))
    before = [x.clone() for x in st]
    new, info = alg.step(prng.key(1), st)
    for x, x0, y in zip(st, before, new):
        assert same_bits(x, x0) and y.data_ptr() != x.data_ptr()
    assert not same_bits(new.position, st.position)
    assert new.position.shape == (N, 4) and new.logdensity.shape == (N,) and info.momentum.shape == (N, 4)
    assert info.theta.shape == (N,) and info.subiter.shape == (N,)
    for k in prng.split(prng.key(7), T):
        st, info = alg.step(k, st)
    mean_se, var_se = moment_errors(t2n(st.position))
    print("mean (s.e.):", mean_se, "var (s.e.):", var_se)
    assert np.all(mean_se <= 5.0), mean_se
    assert np.all(var_se <= 5.0), var_se
    assert same_bits(st.logdensity, loglik(st.position))


def test_ess_cap_on_sub_iterations(dev):
    """The reference's while_loop has no cap; here a transition that cannot end -- the state's logdensity and the
    likelihood are -inf everywhere -- raises after max_subiter likelihood evaluations, and the next ordinary transition
    on a fresh state works."""
    N, D = 8, 4
    calls = []

    def never(q):
        calls.append(1)
        return torch.full((q.shape[0],), float("-inf"), device=q.device)

    alg = bjx.elliptical_slice(never, mean=0.0, cov=torch.ones(D), max_subiter=6)
    st = alg.init(torch.zeros(N, D, device=dev))
    assert bool(torch.isinf(st.logdensity).all())
    calls.clear()
    with pytest.raises(RuntimeError, match="8 of 8 chains"):
        alg.step(prng.key(1), st)
    assert len(calls) == 6

    ok = bjx.elliptical_slice(lambda q: -0.5 * (q * q).sum(-1), mean=0.0, cov=torch.ones(D))
    st2, info = ok.step(prng.key(1), ok.init(torch.zeros(N, D, device=dev)))
    assert bool(torch.isfinite(st2.position).all()) and bool((info.subiter >= 1).all())
    e = ok.step(prng.key(1), ok.init(torch.zeros(0, D, device=dev)))[0]  # an empty batch is a no-op
    assert e.position.shape == (0, D)
