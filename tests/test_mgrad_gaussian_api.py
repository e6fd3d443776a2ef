"""``blackjax_amd.mgrad_gaussian``: API surface, argument errors and the host-side factorisation (no GPU needed), and
the NumPy restatement the GPU tests hold the kernels against (tests/mgrad_gaussian_restatement.py), pinned on its own:
the detailed balance of its formulas and its stationarity on a closed-form posterior."""
import inspect

import numpy as np
import pytest
import torch

import mgrad_gaussian_restatement as rmg
from oracle import prng, targets as otargets

f32 = np.float32


def test_mgrad_api_surface():
    import blackjax_amd as bjx
    from blackjax_amd import marginal_latent_gaussian as mlg

    assert "mgrad_gaussian" in bjx.__all__ and "marginal_latent_gaussian" in bjx.__all__
    assert bjx.marginal_latent_gaussian is mlg
    assert callable(bjx.mgrad_gaussian)
    assert bjx.mgrad_gaussian.init is mlg.init and bjx.mgrad_gaussian.build_kernel is mlg.build_kernel
    assert mlg.MarginalState._fields == ("position", "logdensity", "logdensity_grad", "U_x", "U_grad_x")
    assert mlg.MarginalInfo._fields == ("acceptance_rate", "is_accepted", "proposal")
    assert mlg.CovarianceSVD._fields == ("U", "Gamma", "U_t")
    for name in ("MarginalState", "MarginalInfo", "CovarianceSVD"):
        assert getattr(rmg, name)._fields == getattr(mlg, name)._fields
    for name in ("svd_from_covariance", "generate_mean_shifted_logprob", "init", "build_kernel", "as_top_level_api"):
        assert callable(getattr(mlg, name)) and name in mlg.__all__
    sig = inspect.signature(mlg.as_top_level_api)
    assert [(p.name, p.kind, p.default) for p in sig.parameters.values()] == [
        ("logdensity_fn", inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.empty),
        ("covariance", inspect.Parameter.POSITIONAL_OR_KEYWORD, None),
        ("mean", inspect.Parameter.POSITIONAL_OR_KEYWORD, None),
        ("cov_svd", inspect.Parameter.POSITIONAL_OR_KEYWORD, None),
        ("step_size", inspect.Parameter.POSITIONAL_OR_KEYWORD, 1.0),
        ("chain_offset", inspect.Parameter.KEYWORD_ONLY, 0)]
    assert list(inspect.signature(mlg.init).parameters) == ["position", "logdensity_fn", "U_t"]
    assert list(inspect.signature(mlg.build_kernel).parameters) == ["cov_svd"]
    kernel = mlg.build_kernel(mlg.svd_from_covariance(torch.eye(3)))
    assert list(inspect.signature(kernel).parameters) == ["rng_key", "state", "logdensity_fn", "delta", "chain_offset"]
    alg = bjx.mgrad_gaussian(lambda q: -0.5 * (q * q).sum(-1), covariance=torch.eye(3), step_size=0.5)
    assert isinstance(alg, bjx.SamplingAlgorithm) and callable(alg.init) and callable(alg.step)
    assert "safe_energy_diff" in mlg.__doc__ and "per-chain" in mlg.__doc__ and "diagonal prior" in mlg.__doc__


def test_mgrad_argument_errors_come_before_any_device_check():
    """Everything here is raised with CPU inputs: a CPU position would otherwise be refused with RuntimeError."""
    import blackjax_amd as bjx

    fn = lambda q: -0.5 * (q * q).sum(-1)  # noqa: E731
    D = 4
    cov = torch.eye(D)
    with pytest.raises(ValueError, match="covariance or cov_svd"):
        bjx.mgrad_gaussian(fn)
    with pytest.raises(ValueError):
        bjx.mgrad_gaussian(fn, covariance=cov, mean=torch.zeros(D + 1))  # mean of the wrong length
    with pytest.raises(ValueError):
        bjx.mgrad_gaussian(fn, covariance=torch.ones(D), mean=torch.zeros(D + 1))
    with pytest.raises(ValueError):
        bjx.mgrad_gaussian(fn, covariance=torch.ones(3, 4))  # a 2-d covariance is dense: it must be square
    with pytest.raises(ValueError):
        bjx.mgrad_gaussian(fn, covariance=torch.tensor(1.0))  # 0-d
    with pytest.raises(NotImplementedError):
        bjx.mgrad_gaussian(fn, covariance=torch.ones(2, D, D))  # per-chain priors
    with pytest.raises(NotImplementedError):
        bjx.mgrad_gaussian(fn, covariance=cov, mean=torch.zeros(2, D))  # per-chain means
    indefinite = torch.diag(torch.tensor([1.0, 2.0, -0.5, 1.0]))
    with pytest.raises(ValueError, match="positive definite"):
        bjx.mgrad_gaussian(fn, covariance=indefinite)
    with pytest.raises(ValueError, match="positive definite"):
        bjx.mgrad_gaussian(fn, covariance=torch.tensor([1.0, 0.0, 1.0]))  # a diagonal prior with a zero variance
    with pytest.raises(ValueError, match="positive definite"):
        bjx.marginal_latent_gaussian.svd_from_covariance(torch.zeros(D, D))
    svd = bjx.marginal_latent_gaussian.svd_from_covariance(cov)
    with pytest.raises(ValueError):
        bjx.mgrad_gaussian(fn, cov_svd=svd, mean=torch.zeros(D + 1))
    with pytest.raises(ValueError, match="positive definite"):
        bjx.mgrad_gaussian(fn, cov_svd=svd._replace(Gamma=torch.tensor([1.0, 1.0, 0.0, 1.0])))
    with pytest.raises(ValueError):
        bjx.mgrad_gaussian(fn, cov_svd=svd._replace(U_t=None))
    # position of the wrong width: a shape error, not the device error a CPU tensor would otherwise get
    alg = bjx.mgrad_gaussian(fn, covariance=cov, mean=torch.zeros(D))
    with pytest.raises(ValueError):
        alg.init(torch.zeros(3, D + 1))
    with pytest.raises(ValueError):
        alg.init(torch.zeros(D))
    bad = bjx.marginal_latent_gaussian.MarginalState(*(torch.zeros(3, D + 1),) * 5)
    with pytest.raises(ValueError):
        alg.step(prng.key(0), bad)
    with pytest.raises(RuntimeError):
        alg.init(torch.zeros(3, D))  # and a well-shaped host tensor: there is no CPU fallback


def test_mgrad_entry_points_reject_bad_arguments_without_gpu():
    from blackjax_amd import _lib

    lib = _lib.load()
    tails = {"bjx_mgrad_propose": (None, 1, 2, 0, -1, 4, 8, 0.1, None) + (None,) * 4,
             "bjx_mgrad_shift": (None, 4, 8) + (None,) * 6,
             "bjx_mgrad_finish": (None, 1, 2, 0, -1, 4, 8, 0.1, None) + (None,) * 18}
    for name, args in tails.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == len(args)
        assert getattr(lib, name)(*args) != 0 and name.encode() + b": null pointer" in lib.bjx_last_error()
        n_at = 1 if name == "bjx_mgrad_shift" else 5
        for n, d in ((-1, 8), (4, 0), (4, -3)):  # sizes are checked before the pointers
            a = list(args)
            a[n_at], a[n_at + 1] = n, d
            assert getattr(lib, name)(*a) != 0 and name.encode() + b": bad sizes" in lib.bjx_last_error()
        a = list(args)
        a[n_at] = 0  # an empty batch is a no-op
        assert getattr(lib, name)(*a) == 0
    assert lib.bjx_abi_version() == 7  # additive


def test_svd_from_covariance():
    from blackjax_amd import marginal_latent_gaussian as mlg

    D = 12
    a = prng.normal(prng.key(3), (D, D)).astype(np.float64)
    cov = a @ a.T + 0.25 * np.eye(D)
    svd = mlg.svd_from_covariance(torch.as_tensor(cov))
    U, gamma, U_t = (t.numpy() for t in svd)
    assert U.dtype == f32 and gamma.dtype == f32 and U_t.dtype == f32
    assert svd.U.is_contiguous() and svd.U_t.is_contiguous() and np.array_equal(U_t, U.T)
    assert np.all(np.diff(gamma) <= 0) and gamma[-1] > 0  # descending, as an SVD's
    eps = np.finfo(f32).eps
    # each factor carries one fp32 rounding of entries <= 1 (U) / of Gamma: D terms per product entry
    rec = (U.astype(np.float64) * gamma.astype(np.float64)) @ U_t.astype(np.float64)
    assert np.abs(rec - cov).max() <= 4 * D * eps * np.abs(cov).max()
    assert np.abs(U_t.astype(np.float64) @ U.astype(np.float64) - np.eye(D)).max() <= 4 * D * eps
    # the shift of generate_mean_shifted_logprob is C^-1 mean
    mean = np.linspace(-1.0, 1.0, D)
    shifted = mlg.generate_mean_shifted_logprob(lambda q: q.sum(-1), torch.as_tensor(mean), torch.as_tensor(cov))
    np.testing.assert_allclose(shifted.shift.numpy(), np.linalg.solve(cov, mean), rtol=1e-3, atol=1e-5)
    # a 1-d covariance is a diagonal prior
    diag = mlg.svd_from_covariance(torch.tensor([2.0, 0.5]))
    assert diag.U is None and diag.U_t is None and diag.Gamma.tolist() == [2.0, 0.5]


def _log_normal(v, mean, cov):
    d = v - mean
    return -0.5 * d @ np.linalg.solve(cov, d) - 0.5 * np.linalg.slogdet(2.0 * np.pi * cov)[1]


@pytest.mark.parametrize("delta", [0.1, 1.0, 7.0])
def test_formulas_satisfy_detailed_balance(delta):
    """log_ratio of the transition formulas equals log pi(y) + log q(x | y) - log pi(x) - log q(y | x) computed from
    explicit Gaussian densities (pi = N(0, C) exp(loglik), a non-Gaussian likelihood, D = 7) to 1e-10.  No reference
    source is available: this pins the restatement itself."""
    rng = np.random.default_rng(0)
    D, n = 7, 6
    a = rng.standard_normal((D, D))
    C = a @ a.T + 0.5 * np.eye(D)
    w, U = np.linalg.eigh(C)
    w, U = w[::-1], U[:, ::-1]

    def lik(x):
        return -np.sum(np.log(np.cosh(x)) + 0.1 * x ** 4, -1), -(np.tanh(x) + 0.4 * x ** 3)

    x, y = rng.standard_normal((n, D)), rng.standard_normal((n, D))
    (lx, gx), (ly, gy) = lik(x), lik(y)
    log_ratio = rmg.log_ratio_f64(x, lx, gx, y, ly, gy, U, w, delta)
    mean_x, var = rmg.proposal_moments_f64(x, gx, U, w, delta)
    mean_y, _ = rmg.proposal_moments_f64(y, gy, U, w, delta)
    Q = (U * var) @ U.T
    for i in range(n):
        ref = (_log_normal(y[i], 0.0, C) + ly[i] + _log_normal(x[i], U @ mean_y[i], Q)
               - _log_normal(x[i], 0.0, C) - lx[i] - _log_normal(y[i], U @ mean_x[i], Q))
        assert abs(log_ratio[i] - ref) <= 1e-10, (log_ratio[i], ref)


def test_restatement_matches_its_fp64_formulas():
    """The house-rounded transition agrees with the plain fp64 formulas on its own proposals to fp32 rounding."""
    N, D, delta = 8, 24, 1.5
    svd = rmg.random_factor(D)
    fn = otargets.diag_gaussian(np.linspace(0.5, 2.0, D).astype(f32))
    st = rmg.init(prng.normal(prng.key(1), (N, D)).astype(f32), fn, svd)
    f = lambda a: np.asarray(a, np.float64)  # noqa: E731
    rates = []
    for k in prng.split(prng.key(2), 6):
        new, info = rmg.kernel(k, st, fn, svd, delta)
        p = info.proposal
        lr = rmg.log_ratio_f64(f(st.position), f(st.logdensity), f(st.logdensity_grad), f(p.position),
                               f(p.logdensity), f(p.logdensity_grad), f(svd.U), f(svd.Gamma), delta)
        np.testing.assert_allclose(info.acceptance_rate, np.minimum(1.0, np.exp(lr)), rtol=1e-3)
        rates.append(info.acceptance_rate)
        st = new
    rates = np.concatenate(rates)
    assert np.sum((rates > 0.01) & (rates < 0.99)) >= 8  # the comparison is not of saturated rates only


def test_restatement_is_stationary_on_a_closed_form_posterior():
    """Prior N(mean, U diag(Gamma) U_t) with a non-zero mean, Gaussian likelihood, D = 16, 512 chains, 200
    transitions at delta = 1.0, second half kept (rmg.stationarity_case).  The posterior is Gaussian in closed form;
    the restatement's pooled mean and variances must lie within three times the worst error of the plain fp64
    transition (rmg.stationarity_errors_f64) over five seeds of NumPy's generator.  Those five runs gave, for seeds
    0..4 (max |mean error| / min posterior sd ; max |var ratio - 1| ; mean acceptance):

        0.03779 ; 0.01885 ; 0.481      0.04796 ; 0.01410 ; 0.482      0.03439 ; 0.01666 ; 0.478
        0.04644 ; 0.03057 ; 0.481      0.04190 ; 0.03538 ; 0.481

    so the bounds are 3 * 0.04796 = 0.1439 and 3 * 0.03539 = 0.1062 (rmg.STATIONARITY_MEAN_BOUND / _VAR_BOUND); the
    restatement itself measured 0.0486 and 0.0196 with acceptance 0.482.  (At delta = 0.3 the five fp64 runs gave
    0.055-0.063 and 0.023-0.035 with acceptance 0.863.)  The GPU test runs the same case on the device."""
    case = rmg.stationarity_case()
    delta = rmg.STATIONARITY_DELTA
    assert rmg.STATIONARITY_MEAN_BOUND == 3 * 0.04796 and rmg.STATIONARITY_VAR_BOUND == 3 * 0.03539
    fn = rmg.mean_shifted(otargets.diag_gaussian(case.inv_var), rmg.shift_from_svd(case.cov_svd, case.mean))
    st = rmg.init(case.x0, fn, case.cov_svd)
    kept, rates = [], []
    for t, k in enumerate(prng.split(prng.key(31), case.n_steps)):
        st, info = rmg.kernel(k, st, fn, case.cov_svd, delta)
        if t >= case.n_steps // 2:
            kept.append(st.position)
            rates.append(info.acceptance_rate.mean())
    mean_err, var_err = rmg.stationarity_errors(np.stack(kept), case)
    print("mean error / min sd:", mean_err, "max |var ratio - 1|:", var_err, "acceptance:", float(np.mean(rates)))
    assert mean_err <= rmg.STATIONARITY_MEAN_BOUND, mean_err
    assert var_err <= rmg.STATIONARITY_VAR_BOUND, var_err
    assert 0.3 < float(np.mean(rates)) < 0.7  # both branches of the accept are taken
    lp, g = fn(st.position)
    assert np.array_equal(lp, st.logdensity) and np.array_equal(g, st.logdensity_grad)  # the state is consistent
    np.testing.assert_array_equal(rmg.matmul(st.position, case.cov_svd.U), st.U_x)
