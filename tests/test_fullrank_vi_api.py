"""API surface of fullrank_vi (blackjax_amd/vi/fullrank_vi.py, include/bjx_hip.h "VI") and the arithmetic of its
NumPy restatement, tests/fullrank_vi_restatement.py.  Needs no GPU."""
import inspect

import numpy as np
import pytest
import torch

import blackjax_amd as bjx
import fullrank_vi_restatement as rv
import meanfield_vi_restatement as mrv
from blackjax_amd import _lib, optim
from blackjax_amd.vi import fullrank_vi as frvi
from oracle import prng, targets as otargets

f32, f64 = np.float32, np.float64
T, B = frvi.DRAW_TILE, frvi.COL_BLOCK
# every D of test_fullrank_vi_gpu.py
GPU_DIMS = sorted({1, 3, 4, 8, 16, B - 1, B, B + 1, 2 * B + 3})


def _defaults(fn):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty}


# ----------------------------------------------------------------------------- names and signatures
def test_names_and_signatures():
    assert "fullrank_vi" in bjx.__all__ and "fullrank_vi" in bjx.vi.__all__ and bjx.vi.fullrank_vi is frvi
    assert isinstance(bjx.fullrank_vi, bjx.GenerateVariationalAPI)
    assert bjx.fullrank_vi.init is frvi.init and bjx.fullrank_vi.step is frvi.step
    assert bjx.fullrank_vi.sample is frvi.sample
    for name in ("FRVIState", "FRVIInfo", "init", "step", "sample", "kl_and_grad", "generate_fullrank_logdensity",
                 "cholesky_factor", "as_top_level_api"):
        assert name in frvi.__all__ and hasattr(frvi, name)
    assert frvi.FRVIState._fields == ("mu", "chol_params", "opt_state") and frvi.FRVIInfo._fields == ("elbo",)
    assert list(inspect.signature(frvi.init).parameters) == ["position", "optimizer"]
    assert list(inspect.signature(frvi.step).parameters) == ["rng_key", "state", "logdensity_fn", "optimizer",
                                                             "num_samples", "stl_estimator"]
    assert _defaults(frvi.step) == {"num_samples": 5, "stl_estimator": True}
    assert list(inspect.signature(frvi.sample).parameters) == ["rng_key", "state", "num_samples"]
    assert _defaults(frvi.sample) == {"num_samples": 1}
    assert list(inspect.signature(frvi.kl_and_grad).parameters) == ["rng_key", "mu", "chol_params", "logp", "grad",
                                                                    "stl_estimator"]
    assert _defaults(frvi.kl_and_grad) == {"stl_estimator": True}
    assert list(inspect.signature(frvi.generate_fullrank_logdensity).parameters) == ["mu", "cov"]
    assert list(inspect.signature(frvi.cholesky_factor).parameters) == ["state"]
    assert list(inspect.signature(frvi.as_top_level_api).parameters) == ["logdensity_fn", "optimizer", "num_samples"]
    assert _defaults(frvi.as_top_level_api) == {"num_samples": 100}
    alg = bjx.fullrank_vi(lambda z: -(z * z).sum(-1), optim.adam(0.05))
    assert isinstance(alg, bjx.VIAlgorithm)
    assert list(inspect.signature(alg.init).parameters) == ["position"]
    assert list(inspect.signature(alg.step).parameters) == ["rng_key", "state"]
    assert list(inspect.signature(alg.sample).parameters) == ["rng_key", "state", "num_samples"]
    assert _defaults(alg.sample) == {"num_samples": 1}


def test_host_tensors_are_refused():
    """There is no CPU fallback: parameters on the host raise before anything is launched."""
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frvi.init(torch.zeros(3), optim.adam(0.05))
    state = frvi.FRVIState(torch.zeros(3), torch.zeros(6), None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frvi.sample(prng.key(0), state, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frvi.kl_and_grad(prng.key(0), state.mu, state.chol_params, torch.zeros(2), torch.zeros(2, 3))


def test_entry_points_check_their_arguments():
    lib = _lib.load()
    assert lib.bjx_vi_fullrank_tile() == T and lib.bjx_vi_fullrank_block() == B
    # the supported sizes reach D = 2048 and S = 65 536; the workspace holds the fp64 W, 8 S D bytes, and more
    for S, D in ((1, 1), (T, B), (T + 1, B + 1), (5, 2048), (65536, 2048), (2 ** 20, 128), (2 ** 15, 4096)):
        assert lib.bjx_vi_fullrank_grad_workspace_bytes(S, D) > 8 * S * D
    for S, D in ((0, 4), (4, 0), (2 ** 20 + 1, 1), (1, 4097), (2 ** 20, 256)):
        assert lib.bjx_vi_fullrank_grad_workspace_bytes(S, D) == 0
        assert lib.bjx_vi_fullrank_sample(None, 1, 2, S, D, None, None, None) != 0
        assert b"bjx_vi_fullrank_sample: bad sizes" in lib.bjx_last_error()
        assert lib.bjx_vi_fullrank_grad(None, 1, 2, S, D, 1, None, None, None, None, None, None, None) != 0
        assert b"bjx_vi_fullrank_grad: bad sizes" in lib.bjx_last_error()
    assert lib.bjx_vi_fullrank_grad(None, 1, 2, 4, 4, 2, None, None, None, None, None, None, None) != 0
    assert b"bjx_vi_fullrank_grad: bad sizes" in lib.bjx_last_error()
    assert lib.bjx_vi_fullrank_sample(None, 1, 2, 4, 4, None, None, None) != 0
    assert b"bjx_vi_fullrank_sample: null pointer" in lib.bjx_last_error()
    assert lib.bjx_vi_fullrank_grad(None, 1, 2, 4, 4, 0, None, None, None, None, None, None, None) != 0
    assert b"bjx_vi_fullrank_grad: null pointer" in lib.bjx_last_error()


# ----------------------------------------------------------------------------- the packing
@pytest.mark.parametrize("D", [1, 2, 5, 9])
def test_packing_is_tril_indices_order(D):
    n = rv.num_params(D)
    chol = np.arange(1, n + 1, dtype=f64) / n
    L = rv.unflatten(chol, np.exp(chol[:D]))
    rows, cols = torch.tril_indices(D, D, -1)
    assert np.array_equal(L[rows.numpy(), cols.numpy()], chol[D:])
    for k, (i, j) in enumerate(zip(rows.tolist(), cols.tolist())):
        assert rv.index(D, i, j) == D + k and j < i
    assert [rv.index(D, i, i) for i in range(D)] == list(range(D))
    assert np.array_equal(np.triu(L, 1), np.zeros((D, D))) and np.array_equal(np.diag(L), np.exp(chol[:D]))
    assert np.array_equal(rv.flatten(chol[:D], L), chol)
    # the package's plain PyTorch helpers use the same packing
    Lt = frvi._unflatten_cholesky(torch.as_tensor(chol))
    np.testing.assert_allclose(Lt.numpy(), L, rtol=1e-15, atol=0)
    state = frvi.FRVIState(torch.zeros(D, dtype=torch.float64), torch.as_tensor(chol), None)
    assert torch.equal(frvi.cholesky_factor(state), Lt)
    with pytest.raises(ValueError, match="chol_params must be"):
        frvi._unflatten_cholesky(torch.zeros(n + 1))


# ----------------------------------------------------------------------------- the formulas against autograd
def _reference_unflatten(chol_params, D):
    """The reference's ``_unflatten_cholesky``: ``tril_indices(D, k=-1)`` filled from the tail, ``exp`` of the head on
    the diagonal."""
    L = torch.zeros(D, D, dtype=chol_params.dtype)
    rows, cols = torch.tril_indices(D, D, -1)
    L = L.index_put((rows, cols), chol_params[D:])
    return L + torch.diag(torch.exp(chol_params[:D]))


@pytest.mark.parametrize("stl", [True, False])
@pytest.mark.parametrize("S,D", [(4, 1), (6, 2), (7, 5)])
def test_gradient_formulas_match_autograd_of_the_reference_lines(S, D, stl):
    """The restatement's formulas against ``torch.autograd`` in fp64 of the reference's literal lines:
    ``_unflatten_cholesky``, ``z = eps @ L.T + mu``, ``multivariate_normal.logpdf(z, mu, L L^T)`` with the parameters
    detached under STL, ``kl = (logq - logp).mean()``.  The target is a non-Gaussian function, so that ``G`` depends on
    ``z``."""
    rng = np.random.default_rng(10 * S + D)
    eps = torch.as_tensor(prng.normal(prng.key(S + D), (S, D)).astype(f64))
    mu = torch.as_tensor(rng.standard_normal(D), dtype=torch.float64).requires_grad_(True)
    chol0 = np.concatenate([rng.uniform(-1.5, 0.5, D), rng.standard_normal(rv.num_params(D) - D) * 0.5])
    chol = torch.as_tensor(chol0, dtype=torch.float64).requires_grad_(True)
    a, b = torch.as_tensor(rng.standard_normal(D)), torch.as_tensor(rng.uniform(0.5, 2.0, D))

    def logp_fn(z):
        return (-0.5 * b * (z - a) ** 2 + torch.sin(z)).sum(-1) + 0.1 * z.prod(-1)

    L = _reference_unflatten(chol, D)
    z = eps @ L.T + mu
    mu_q, L_q = (mu.detach(), L.detach()) if stl else (mu, L)
    logq = torch.distributions.MultivariateNormal(mu_q, covariance_matrix=L_q @ L_q.T).log_prob(z)
    kl = (logq - logp_fn(z)).mean()
    g_mu, g_chol = torch.autograd.grad(kl, (mu, chol))

    zd = z.detach().requires_grad_(True)
    logp = logp_fn(zd)
    (G,) = torch.autograd.grad(logp.sum(), zd)
    kl_r, g_mu_r, g_chol_r = rv.kl_and_grad_terms(eps.numpy(), L.detach().numpy(), chol0[:D], logp.detach().numpy(),
                                                  G.numpy(), stl)
    assert g_chol_r.shape == (rv.num_params(D),)
    np.testing.assert_allclose(kl_r, kl.item(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(g_mu_r, g_mu.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(g_chol_r, g_chol.numpy(), rtol=1e-12, atol=1e-12)
    # the approximation's log-density: the closed form, and as the package forms it
    cov = (L @ L.T).detach()
    np.testing.assert_allclose(rv.fullrank_logdensity(mu.detach().numpy(), cov.numpy(), z.detach().numpy()),
                               logq.detach().numpy(), rtol=1e-12, atol=1e-12)
    ld = frvi.generate_fullrank_logdensity(mu.detach(), cov)(z.detach())
    assert ld.shape == (S,)
    np.testing.assert_allclose(ld.numpy(), logq.detach().numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("stl", [True, False])
def test_zero_strict_lower_triangle_is_meanfield(stl):
    """With a zero strict lower triangle the restatement is meanfield_vi_restatement's with ``rho`` the log-diagonal:
    the draws, ``kl``, ``g_mu`` and ``g_chol[:D]`` against ``g_rho``.  The strict-lower gradient is not zero."""
    S, D = 7, 5
    rng = np.random.default_rng(1)
    key = prng.key(2)
    mu, rho = rng.standard_normal(D).astype(f32), rng.uniform(-1.5, 0.5, D).astype(f32)
    chol = np.concatenate([rho, np.zeros(rv.num_params(D) - D, f32)])
    logp, G = rng.standard_normal(S).astype(f32), rng.standard_normal((S, D)).astype(f32)
    np.testing.assert_allclose(rv.sample(key, mu, chol, S), mrv.sample(key, mu, rho, S), rtol=1e-7, atol=0)
    kl, g_mu, g_chol = rv.kl_and_grad(key, mu, chol, logp, G, stl)
    kl_m, g_mu_m, g_rho_m = mrv.kl_and_grad(key, mu, rho, logp, G, stl)
    np.testing.assert_allclose(kl, kl_m, rtol=1e-13)
    np.testing.assert_allclose(g_mu, g_mu_m, rtol=1e-13, atol=1e-14)
    np.testing.assert_allclose(g_chol[:D], g_rho_m, rtol=1e-13, atol=1e-14)
    assert np.abs(g_chol[D:]).min() > 0


def test_restated_sample_and_step_are_consistent():
    """``sample`` is ``mu + L eps`` on the draws of the key itself, rounded once; ``step`` draws what ``sample`` returns
    and applies the restated Adam to the rounded gradients; ``init`` is ``mu = 0``, ``L = I``."""
    S, D = 7, 4
    key = prng.key(5)
    mu, chol = rv.factor_case(D)
    z = rv.sample(key, mu, chol, S)
    eps = prng.normal(key, (S, D)).astype(f64)
    L = rv.unflatten(chol)
    assert z.dtype == f32 and z.shape == (S, D)
    assert np.array_equal(np.diag(L), np.exp(chol[:D].astype(f64)).astype(f32))
    want = np.array([[mu[i] + sum(L[i, j] * eps[s, j] for j in range(i + 1)) for i in range(D)] for s in range(S)])
    np.testing.assert_allclose(z, want, rtol=1e-7, atol=0)
    u = rv.back_substitute(L, eps)
    np.testing.assert_allclose(u @ L, eps, rtol=1e-12, atol=1e-13)  # L^T u_s = eps_s, row by row
    opt = rv.Adam(0.05)
    state = rv.FRVIState(mu, chol, opt.init((mu, chol)))
    fn = otargets.ar1_gaussian(0.9, D)
    new, kl = rv.step(key, state, fn, opt, S)
    logp, G = fn(z)
    kl_r, g_mu, g_chol = rv.kl_and_grad(key, mu, chol, logp, G)
    upd, _ = opt.update((g_mu.astype(f32), g_chol.astype(f32)), state.opt_state)
    assert kl == f32(kl_r) and new.opt_state.count == 1
    assert np.array_equal(new.mu, mu + upd[0]) and np.array_equal(new.chol_params, chol + upd[1])
    first = rv.init(np.full(D, 3.0, f32), opt)
    assert not first.mu.any() and not first.chol_params.any() and first.chol_params.shape == (rv.num_params(D),)
    assert np.array_equal(rv.unflatten(first.chol_params), np.eye(D))


# ----------------------------------------------------------------------------- the factors of the GPU tests
def test_gpu_test_factors_are_well_conditioned():
    """The Cholesky factors of test_fullrank_vi_gpu.py (``factor_case``) have condition number below 100 at every ``D``
    used there (27 at most), and on them the restatement's fp64 back-substitution differs from one in ``longdouble``
    summed in the opposite order by less than 1e-12 relative: the solve's own error is far inside RTOL = 1e-6."""
    for D in GPU_DIMS:
        mu, chol = rv.factor_case(D)
        assert mu.shape == (D,) and chol.shape == (rv.num_params(D),) and chol.dtype == f32
        L = rv.unflatten(chol)
        cond = np.linalg.cond(L)
        assert cond < 100, (D, cond)
        eps = prng.normal(prng.key(D), (5, D)).astype(f64)
        U = rv.back_substitute(L, eps)
        Ll, el = L.astype(np.longdouble), eps.astype(np.longdouble)
        Ul = np.zeros_like(el)
        for j in range(D - 1, -1, -1):
            acc = el[:, j].copy()
            for i in range(j + 1, D):  # ascending i: the kernels and the restatement go down
                acc -= Ll[i, j] * Ul[:, i]
            Ul[:, j] = acc / Ll[j, j]
        err = float(np.max(np.abs(U - Ul)) / np.max(np.abs(Ul)))
        assert err < 1e-12, (D, err)


# ----------------------------------------------------------------------------- the full-step keys, convergence
def test_full_step_keys_keep_every_gradient_away_from_zero():
    """The keys of test_fullrank_vi_gpu.py's full-step cases: in the restatement no coordinate of either gradient is
    below 1e-4 in magnitude at any of the four steps, so no coordinate is left out of that comparison."""
    assert set(rv.FULL_CASES) == {(5, 3), (32, 16), (40, B + 1)}
    for (S, D) in rv.FULL_CASES:
        keys = rv.full_case(S, D)
        fn, opt = otargets.ar1_gaussian(rv.FULL_RHO, D), rv.Adam(rv.FULL_LR)
        state = rv.init(np.zeros(D, f32), opt)
        for k in keys:
            logp, G = fn(rv.sample(k, state.mu, state.chol_params, S))
            _, g_mu, g_chol = rv.kl_and_grad(k, state.mu, state.chol_params, logp, G)
            assert min(np.abs(g_mu).min(), np.abs(g_chol).min()) >= 1e-4, (S, D)
            state, _ = rv.step(k, state, fn, opt, S)


def test_restated_sampler_converges_on_the_correlated_gaussian():
    """The convergence case (the AR(1) Gaussian with correlation 0.9 in D = 8 about a shifted mean, S = 32, adam(0.05),
    600 steps) in the restatement.  With STL the estimator's variance vanishes at the optimum and the run ends at the
    rounding floor recorded in the restatement (worst of the five keys of ``CONV_SEEDS``: max|mu - m| = 9.54e-7 and
    max|L L^T - C| = 1.23e-6); without STL the same run stays more than 1e-2 from the mean (the five runs ended 0.033
    to 0.074 from m), which shows the flag to act."""
    seed = rv.CONV_SEEDS[0]
    err_mu, err_cov, _ = rv.converge(seed, True)
    print("restatement, STL:", err_mu, err_cov)
    assert err_mu <= rv.CONV_MU_BOUND and err_cov <= rv.CONV_COV_BOUND
    err_mu, err_cov, _ = rv.converge(seed, False)
    print("restatement, no STL:", err_mu, err_cov)
    assert err_mu > 1e-2
