"""GPU parity of the marginal latent-Gaussian sampler (blackjax_amd/marginal_latent_gaussian.py,
csrc/bjx_mgrad.hip, include/bjx_hip.h "marginal latent Gaussian") against the NumPy restatement of the reference's
arithmetic, tests/mgrad_gaussian_restatement.py.  Tolerances of tests/test_mala_gpu.py: accept bits exact, state
arrays (U_x, U_grad_x and info.proposal included) within 1e-6 rtol / atol, acceptance rates within rtol 1e-5.

The step size of every case was chosen with the restatement on the CPU so that 0 < n_accepted < n_transitions * N
(both branches of the select ran); the cases assert it."""
import numpy as np
import pytest
import torch

import blackjax_amd as bjx
import mgrad_gaussian_restatement as rmg
from blackjax_amd import marginal_latent_gaussian as mlg
from oracle import prng, targets as otargets

pytestmark = pytest.mark.gpu
f32 = np.float32


def t2n(t):
    return t.detach().cpu().numpy()


def dev_t(a, dev):
    return torch.as_tensor(np.asarray(a), device=dev)


def same_bits(a, b):
    if a.dtype == torch.float32:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def _dev_svd(svd, dev):
    return mlg.CovarianceSVD(*(None if a is None else dev_t(a, dev) for a in svd))


def _case(N, D, per_chain, delta, diagonal=False):
    """Prior factor (random_factor: U from a QR, Gamma = 10^linspace(-1, 1, D); diagonal: U = None), likelihood
    sigma_j = 10^(-0.5 + j / (D - 1)), start normal(key(1)), ``delta`` times uniform(0.6, 1.6) per chain."""
    svd = rmg.random_factor(D)
    if diagonal:
        svd = rmg.CovarianceSVD(None, svd.Gamma, None)
    sig = (10.0 ** (-0.5 + 1.0 * np.arange(D) / max(D - 1, 1))).astype(f32)
    inv_var = (f32(1) / (sig * sig)).astype(f32)
    x0 = prng.normal(prng.key(1), (N, D)).astype(f32)
    delta = f32(delta)
    if per_chain:
        delta = (delta * np.random.default_rng(100 * N + D).uniform(0.6, 1.6, N)).astype(f32)
    return svd, inv_var, x0, delta


def _assert_state(st_g, st_r):
    for name, a, b in zip(st_r._fields, st_g, st_r):
        np.testing.assert_allclose(t2n(a), b, rtol=1e-6, atol=1e-6, err_msg=name)


def _assert_info(info_g, info_r):
    assert info_g.is_accepted.dtype == torch.bool and info_g.acceptance_rate.dtype == torch.float32
    assert np.array_equal(t2n(info_g.is_accepted), info_r.is_accepted)
    np.testing.assert_allclose(t2n(info_g.acceptance_rate), info_r.acceptance_rate, rtol=1e-5, atol=1e-7)
    _assert_state(info_g.proposal, info_r.proposal)


def _run_parity(dev, svd, fn_g, fn_r, x0, delta, per_chain, n_steps, mean=None, chain_offset=3):
    alg = bjx.mgrad_gaussian(fn_g, cov_svd=_dev_svd(svd, dev), mean=None if mean is None else dev_t(mean, dev),
                             step_size=dev_t(delta, dev) if per_chain else float(delta), chain_offset=chain_offset)
    if mean is not None:
        fn_r = rmg.mean_shifted(fn_r, rmg.shift_from_svd(svd, mean))
    st_g = alg.init(dev_t(x0, dev))
    st_r = rmg.init(x0, fn_r, svd)
    _assert_state(st_g, st_r)
    n_acc = 0
    for k in prng.split(prng.key(9), n_steps):
        st_r, info_r = rmg.kernel(k, st_r, fn_r, svd, delta, chain_offset=chain_offset)
        st_g, info_g = alg.step(k, st_g)
        _assert_info(info_g, info_r)
        _assert_state(st_g, st_r)
        n_acc += int(info_r.is_accepted.sum())
    assert 0 < n_acc < n_steps * x0.shape[0]  # both branches of the select were exercised at this shape
    return st_g, st_r


# (N, D, per-chain delta, delta, transitions): one element; 4-byte sweep; 16-byte resident NI = 1 (scalar / per-chain
# delta); 4-byte sweep beyond one 256-float span; resident NI = 2; one whole 128-row GEMM tile plus ragged rows;
# resident NI = 4 at its largest row; 16-byte two-pass just past the resident limit; N D > 2^19, where the GEMMs leave
# the skinny kernel for the tile kernel
DENSE_CASES = [(5, 1, False, 0.25, 4), (37, 10, True, 0.25, 4), (16, 64, False, 0.25, 4), (24, 64, True, 0.25, 4),
               (7, 259, True, 0.25, 4), (33, 260, True, 0.25, 4), (130, 128, False, 0.25, 4), (9, 1024, True, 0.25, 4),
               (6, 1032, False, 0.25, 4), (2176, 256, True, 0.5, 2)]


@pytest.mark.parametrize("N,D,per_chain,delta,n_steps", DENSE_CASES)
def test_mgrad_dense_transitions_match_restatement(dev, N, D, per_chain, delta, n_steps):
    """init + consecutive transitions without re-sync, chain_offset = 3, dense prior."""
    svd, inv_var, x0, delta = _case(N, D, per_chain, delta)
    _run_parity(dev, svd, bjx.targets.DiagGaussian(dev_t(inv_var, dev)), otargets.diag_gaussian(inv_var), x0, delta,
                per_chain, n_steps)


# 4-byte sweep; resident NI = 1, 2, 4 (the last at its largest row); 16-byte two-pass: every form of the finish
# without the position / gradient pair of a dense prior
@pytest.mark.parametrize("N,D,per_chain,delta", [(37, 10, True, 2.0), (24, 64, True, 1.0), (33, 260, True, 0.25),
                                                 (9, 1024, True, 0.5), (6, 1032, False, 0.25)])
def test_mgrad_diagonal_prior_matches_restatement(dev, N, D, per_chain, delta):
    """A 1-d covariance: U = I, no GEMM, and no eigenbasis copy -- state.U_x shares storage with state.position."""
    svd, inv_var, x0, delta = _case(N, D, per_chain, delta, diagonal=True)
    st_g, _ = _run_parity(dev, svd, bjx.targets.DiagGaussian(dev_t(inv_var, dev)), otargets.diag_gaussian(inv_var),
                          x0, delta, per_chain, 4)
    assert st_g.U_x.data_ptr() == st_g.position.data_ptr()
    assert st_g.U_grad_x.data_ptr() == st_g.logdensity_grad.data_ptr()
    # the same through covariance=(D,)
    alg = bjx.mgrad_gaussian(bjx.targets.DiagGaussian(dev_t(inv_var, dev)), covariance=dev_t(svd.Gamma, dev),
                             step_size=dev_t(delta, dev) if per_chain else float(delta), chain_offset=3)
    st = alg.init(dev_t(x0, dev))
    assert st.U_x.data_ptr() == st.position.data_ptr()
    for k in prng.split(prng.key(9), 4):
        st, info = alg.step(k, st)
        assert info.proposal.U_x.data_ptr() == info.proposal.position.data_ptr()
    for a, b in zip(st, st_g):
        assert same_bits(a, b)
    assert st.U_x.data_ptr() == st.position.data_ptr()


@pytest.mark.parametrize("N,D,diagonal,delta", [(24, 64, False, 0.25), (37, 10, True, 2.0)])
def test_mgrad_mean_shift(dev, N, D, diagonal, delta):
    """A non-zero (D,) prior mean: logdensity / logdensity_grad are the shifted function's, and ``covariance=`` gives
    the bits of ``cov_svd=`` + ``mean`` when the factor is the same fp32 arrays."""
    svd, inv_var, x0, delta = _case(N, D, True, delta, diagonal=diagonal)
    mean = np.linspace(-1.0, 2.0, D).astype(f32)
    fn_g, fn_r = bjx.targets.DiagGaussian(dev_t(inv_var, dev)), otargets.diag_gaussian(inv_var)
    st_g, st_r = _run_parity(dev, svd, fn_g, fn_r, x0, delta, True, 4, mean=mean)
    lp, g = rmg.mean_shifted(fn_r, rmg.shift_from_svd(svd, mean))(st_r.position)
    np.testing.assert_allclose(t2n(st_g.logdensity), lp, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(t2n(st_g.logdensity_grad), g, rtol=1e-6, atol=1e-6)
    lp0, g0 = fn_r(st_r.position)
    assert not np.allclose(lp, lp0) and not np.allclose(g, g0)  # the shift is not a no-op here

    # covariance= against cov_svd= of the same factor
    if diagonal:
        cov = torch.as_tensor(svd.Gamma)
    else:
        cov = torch.as_tensor((svd.U.astype(np.float64) * svd.Gamma.astype(np.float64)) @ svd.U.astype(np.float64).T)
    factor = mlg.svd_from_covariance(cov)
    runs = []
    for kw in (dict(covariance=cov), dict(cov_svd=factor)):
        alg = bjx.mgrad_gaussian(fn_g, mean=torch.as_tensor(mean), step_size=dev_t(delta, dev), chain_offset=3, **kw)
        st = alg.init(dev_t(x0, dev))
        for k in prng.split(prng.key(9), 4):
            st, info = alg.step(k, st)
        runs.append(tuple(st) + (info.acceptance_rate, info.is_accepted))
    for a, b in zip(*runs):
        assert same_bits(a, b)


@pytest.mark.parametrize("delta", [2.0, 8.0])
def test_mgrad_funnel_non_finite_proposals(dev, delta):
    """Neal's funnel as the likelihood with large steps: proposals whose log-density or ratio is not finite are
    rejected with an acceptance rate of exactly 0 (never NaN), as safe_energy_diff prescribes; the state stays
    finite.  The start is 25 * normal: the restatement finds no non-finite proposal from a narrower start at any step
    size (the likelihood's gradient pushes the funnel's neck coordinate up, away from the overflow of e^-y), and from
    this one 5 / 10 of the 320 proposals at delta = 2 / 8 have a log-density of -inf while the start itself is
    finite."""
    N, D = 64, 8
    svd = rmg.random_factor(D)
    x0 = (25.0 * prng.normal(prng.key(2), (N, D))).astype(f32)
    fn_r = otargets.neal_funnel()
    alg = bjx.mgrad_gaussian(bjx.targets.NealFunnel(), cov_svd=_dev_svd(svd, dev), step_size=delta)
    st_g = alg.init(dev_t(x0, dev))
    st_r = rmg.init(x0, fn_r, svd)
    n_acc = n_zero = n_nonfinite = 0
    for k in prng.split(prng.key(4), 5):
        st_r, info_r = rmg.kernel(k, st_r, fn_r, svd, delta)
        st_g, info_g = alg.step(k, st_g)
        rate = t2n(info_g.acceptance_rate)
        assert np.array_equal(t2n(info_g.is_accepted), info_r.is_accepted)
        assert not np.isnan(rate).any()
        assert np.all(rate[info_r.acceptance_rate == 0] == 0)
        for x in st_g:
            assert bool(torch.isfinite(x).all())
        n_acc += int(info_r.is_accepted.sum())
        n_zero += int((info_r.acceptance_rate == 0).sum())
        n_nonfinite += int((~np.isfinite(info_r.proposal.logdensity)
                            | ~np.isfinite(info_r.proposal.logdensity_grad).all(-1)).sum())
    # the case does contain accepted, rejected and non-finite proposals
    assert 0 < n_acc < 5 * N and n_zero > 0 and n_nonfinite > 0


def test_mgrad_is_shard_invariant_and_chain_major(dev):
    """Chains are keyed by their GLOBAL index: chains [0, 10) and [10, 24) run with chain_offset 3 and 13 reproduce
    the unsplit run bit for bit, state and info.  A chain-major key through run_inference_algorithm equals the
    restatement driven with chain i's keys split(split(key, .)[3 + i], .)[t]."""
    N, D = 24, 64
    svd, inv_var, x0, delta = _case(N, D, True, 0.25)
    fn = bjx.targets.DiagGaussian(dev_t(inv_var, dev))
    svd_g, x0_g, delta_g = _dev_svd(svd, dev), dev_t(x0, dev), dev_t(delta, dev)

    def run(lo, hi):
        alg = bjx.mgrad_gaussian(fn, cov_svd=svd_g, step_size=delta_g[lo:hi].contiguous(), chain_offset=3 + lo)
        st = alg.init(x0_g[lo:hi].contiguous())
        for k in prng.split(prng.key(9), 4):
            st, info = alg.step(k, st)
        return tuple(st) + (info.acceptance_rate, info.is_accepted) + tuple(info.proposal)

    full, a, b = run(0, N), run(0, 10), run(10, N)
    for f, x, y in zip(full, a, b):
        assert same_bits(f, torch.cat([x, y]))

    T = 4
    alg = bjx.mgrad_gaussian(fn, cov_svd=svd_g, step_size=delta_g, chain_offset=3)
    st_g, (hist_state, hist_info) = bjx.util.run_inference_algorithm(prng.key(21), alg, T, initial_state=alg.init(x0_g),
                                                                     key_layout="chain_major")
    fn_r = otargets.diag_gaussian(inv_var)
    st_r = rmg.init(x0, fn_r, svd)
    chain_keys = prng.split(prng.key(21), N, offset=3)
    for t in range(T):
        st_r, info_r = rmg.kernel(None, st_r, fn_r, svd, delta,
                                  chain_keys_override=prng.split(chain_keys, 1, offset=t)[:, 0])
        assert np.array_equal(t2n(hist_info.is_accepted[t]), info_r.is_accepted)
        np.testing.assert_allclose(t2n(hist_state.position[t]), st_r.position, rtol=1e-6, atol=1e-6)
    _assert_state(st_g, st_r)
    # and the chain-major transitions differ from the step-major ones of the same key
    st_s, _ = alg.step(prng.key(21), alg.init(x0_g))
    assert not torch.equal(st_s.position, hist_state.position[0])


def test_mgrad_plain_pytorch_logdensity(dev):
    """A plain PyTorch function handed to ``mgrad_gaussian(...)`` as is gives the accept bits of
    ``targets.DiagGaussian``; positions agree within 1e-6."""
    N, D = 16, 64
    svd, inv_var, x0, delta = _case(N, D, False, 0.25)
    iv = dev_t(inv_var, dev)
    svd_g = _dev_svd(svd, dev)
    alg_p = bjx.mgrad_gaussian(lambda q: -(0.5 * iv * q * q).sum(-1), cov_svd=svd_g, step_size=float(delta))
    alg_t = bjx.mgrad_gaussian(bjx.targets.DiagGaussian(iv), cov_svd=svd_g, step_size=float(delta))
    st_p, st_t = alg_p.init(dev_t(x0, dev)), alg_t.init(dev_t(x0, dev))
    n_acc = 0
    for k in prng.split(prng.key(9), 4):
        st_p, info_p = alg_p.step(k, st_p)
        st_t, info_t = alg_t.step(k, st_t)
        assert torch.equal(info_p.is_accepted, info_t.is_accepted)
        n_acc += int(info_t.is_accepted.sum())
    assert 0 < n_acc < 4 * N
    np.testing.assert_allclose(t2n(st_p.position), t2n(st_t.position), rtol=1e-6, atol=1e-6)


def test_mgrad_stationary_on_the_device(dev):
    """The Gaussian-likelihood case of tests/test_mgrad_gaussian_api.py (D = 16, N = 512, 200 transitions, second half
    kept, non-zero prior mean) stays within the bound recorded there; the accept bits of the first 5 transitions are
    the restatement's."""
    case = rmg.stationarity_case()
    delta = rmg.STATIONARITY_DELTA
    alg = bjx.mgrad_gaussian(bjx.targets.DiagGaussian(dev_t(case.inv_var, dev)), cov_svd=_dev_svd(case.cov_svd, dev),
                             mean=dev_t(case.mean, dev), step_size=delta)
    fn_r = rmg.mean_shifted(otargets.diag_gaussian(case.inv_var), rmg.shift_from_svd(case.cov_svd, case.mean))
    st_g = alg.init(dev_t(case.x0, dev))
    st_r = rmg.init(case.x0, fn_r, case.cov_svd)
    kept = []
    for t, k in enumerate(prng.split(prng.key(31), case.n_steps)):
        st_g, info_g = alg.step(k, st_g)
        if t < 5:
            st_r, info_r = rmg.kernel(k, st_r, fn_r, case.cov_svd, delta)
            assert np.array_equal(t2n(info_g.is_accepted), info_r.is_accepted)
        if t >= case.n_steps // 2:
            kept.append(st_g.position)
    mean_err, var_err = rmg.stationarity_errors(t2n(torch.stack(kept)), case)
    print("mean error / min sd:", mean_err, "max |var ratio - 1|:", var_err)
    assert mean_err <= rmg.STATIONARITY_MEAN_BOUND, mean_err
    assert var_err <= rmg.STATIONARITY_VAR_BOUND, var_err
