"""``blackjax_amd.sgld`` / ``sghmc`` / ``sgnht`` / ``sgmcmc``: API surface, argument errors (no GPU needed), the
gradient helpers on CPU tensors, and the NumPy restatement the GPU tests hold the kernels against
(tests/sgmcmc_restatement.py), pinned on its own as three samplers."""
import inspect
import re
import os

import numpy as np
import pytest
import torch

import sgmcmc_restatement as rsg
from oracle import prng

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_STAT, D_STAT = 4096, 8
SE_REL = np.sqrt(2.0 / (N_STAT * D_STAT))  # relative s.e. of a variance estimated from N * D independent normals


def exact_gradient(q, minibatch):
    """Target N(0, 1) per dimension: g = -q, no minibatch noise."""
    return -q


def _params(fn):
    return [(p.name, p.kind, p.default) for p in inspect.signature(fn).parameters.values()]


def test_sgmcmc_exports_and_signatures():
    import blackjax_amd as bjx
    from blackjax_amd import _lib

    P, K, E = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.empty
    for name in ("sgld", "sghmc", "sgnht", "sgmcmc"):
        assert name in bjx.__all__ and hasattr(bjx, name)
    assert inspect.ismodule(bjx.sgmcmc)
    for mod in ("sgld", "sghmc", "sgnht", "diffusions", "gradients"):
        assert inspect.ismodule(getattr(bjx.sgmcmc, mod))
    for api, mod in ((bjx.sgld, bjx.sgmcmc.sgld), (bjx.sghmc, bjx.sgmcmc.sghmc), (bjx.sgnht, bjx.sgmcmc.sgnht)):
        assert isinstance(api, bjx.GenerateSamplingAPI)
        assert api.init is mod.init and api.build_kernel is mod.build_kernel and api.differentiable is mod.as_top_level_api
    assert bjx.sgmcmc.sgnht.SGNHTState._fields == rsg.SGNHTState._fields == ("position", "momentum", "xi")

    assert _params(bjx.sgld.init) == [("position", P, E)]
    assert _params(bjx.sgld.build_kernel) == []
    assert _params(bjx.sgld.build_kernel()) == [
        ("rng_key", P, E), ("position", P, E), ("grad_estimator", P, E), ("minibatch", P, E), ("step_size", P, E),
        ("temperature", P, 1.0), ("chain_offset", K, 0)]
    assert _params(bjx.sgld.differentiable) == [("grad_estimator", P, E), ("chain_offset", K, 0)]

    assert _params(bjx.sghmc.init) == [("position", P, E)]
    assert _params(bjx.sghmc.build_kernel) == [("alpha", P, 0.01), ("beta", P, 0.0)]
    assert _params(bjx.sghmc.build_kernel()) == [
        ("rng_key", P, E), ("position", P, E), ("grad_estimator", P, E), ("minibatch", P, E), ("step_size", P, E),
        ("num_integration_steps", P, E), ("temperature", P, 1.0), ("chain_offset", K, 0)]
    assert _params(bjx.sghmc.differentiable) == [
        ("grad_estimator", P, E), ("num_integration_steps", P, 10), ("alpha", P, 0.01), ("beta", P, 0.0),
        ("chain_offset", K, 0)]

    assert _params(bjx.sgnht.init) == [("position", P, E), ("rng_key", P, E), ("xi", P, E), ("chain_offset", K, 0)]
    assert _params(bjx.sgnht.build_kernel) == [("alpha", P, 0.01), ("beta", P, 0.0)]
    assert _params(bjx.sgnht.build_kernel()) == [
        ("rng_key", P, E), ("state", P, E), ("grad_estimator", P, E), ("minibatch", P, E), ("step_size", P, E),
        ("temperature", P, 1.0), ("chain_offset", K, 0)]
    assert _params(bjx.sgnht.differentiable) == [
        ("grad_estimator", P, E), ("alpha", P, 0.01), ("beta", P, 0.0), ("chain_offset", K, 0)]

    for api in (bjx.sgld, bjx.sghmc, bjx.sgnht):
        alg = api(exact_gradient)
        assert isinstance(alg, bjx.SamplingAlgorithm)
        assert _params(alg.step) == [("rng_key", P, E), ("state", P, E), ("minibatch", P, E), ("step_size", P, E),
                                     ("temperature", P, 1.0)]
    assert _params(bjx.sgld(exact_gradient).init) == _params(bjx.sghmc(exact_gradient).init) == [
        ("position", P, E), ("rng_key", P, None)]
    assert _params(bjx.sgnht(exact_gradient).init) == [("position", P, E), ("rng_key", P, E), ("init_xi", P, None)]

    header = open(os.path.join(ROOT, "include", "bjx_hip.h")).read()
    assert "SGMCMC" in header
    for name in ("bjx_sgld_step", "bjx_sghmc_step", "bjx_sgnht_step"):
        assert re.search(r"\bint " + name + r"\(", header) and name in _lib.SIGNATURES


def test_sgmcmc_entry_points_reject_bad_arguments_without_gpu():
    from blackjax_amd import _lib

    lib = _lib.load()
    tail = {"bjx_sgld_step": (0.1, None, 1.0, None) + (None,) * 3,
            "bjx_sghmc_step": (0, 0.01, 0.0, 0.1, None, 1.0, None) + (None,) * 5,
            "bjx_sgnht_step": (0.01, 0.0, 0.1, None, 1.0, None) + (None,) * 7}
    for name, args in tail.items():
        fn = getattr(lib, name)
        assert fn(None, 1, 2, 0, -1, 4, 8, *args) != 0 and name.encode() + b": null pointer" in lib.bjx_last_error()
        for n, d in ((-1, 8), (4, 0), (4, -3)):  # sizes are checked before the pointers
            assert fn(None, 1, 2, 0, -1, n, d, *args) != 0 and name.encode() + b": bad sizes" in lib.bjx_last_error()
        assert fn(None, 1, 2, 0, -1, 0, 8, *args) == 0  # an empty batch is a no-op


def test_sgmcmc_argument_errors():
    import blackjax_amd as bjx

    q = torch.zeros(6, 4)  # a host tensor: there is no CPU fallback
    key = prng.key(0)
    with pytest.raises(RuntimeError):
        bjx.sgld(exact_gradient).step(key, q, None, 0.1)
    with pytest.raises(RuntimeError):
        bjx.sgld.init(q)
    with pytest.raises(RuntimeError):
        bjx.sghmc(exact_gradient, 3).step(key, q, None, 0.1)
    with pytest.raises(RuntimeError):
        bjx.sgnht(exact_gradient).init(q, key)
    state = bjx.sgmcmc.sgnht.SGNHTState(q, torch.zeros(6, 4), torch.zeros(6))
    with pytest.raises(RuntimeError):
        bjx.sgnht(exact_gradient).step(key, state, None, 0.1)

    steps = {"sgld": lambda **kw: bjx.sgld(exact_gradient).step(key, q, None, **kw),
             "sghmc": lambda **kw: bjx.sghmc(exact_gradient, 3).step(key, q, None, **kw),
             "sgnht": lambda **kw: bjx.sgnht(exact_gradient).step(key, state, None, **kw)}
    for name, step in steps.items():
        with pytest.raises(ValueError, match="step_size"):
            step(step_size=torch.full((7,), 0.1))  # per-chain step size of the wrong length
        with pytest.raises(ValueError, match="temperature"):
            step(step_size=0.1, temperature=torch.ones(5))
    with pytest.raises(ValueError):
        bjx.sgld(exact_gradient).step(key, torch.zeros(4), None, 0.1)  # not (n_chains, dim)

    for L in (0, -2):
        with pytest.raises(ValueError, match="num_integration_steps"):
            bjx.sghmc(exact_gradient, L).step(key, q, None, 0.1)
    # 2 alpha - eps beta < 0: the reference silently produces NaN
    with pytest.raises(ValueError, match="alpha"):
        bjx.sghmc(exact_gradient, 3, alpha=0.1, beta=1.0).step(key, q, None, 0.3)
    with pytest.raises(ValueError, match="alpha"):
        bjx.sgnht(exact_gradient, alpha=0.1, beta=1.0).step(key, state, None, 0.3)
    with pytest.raises(RuntimeError):  # 2 alpha - eps beta = 0 is allowed: the next check is the device
        bjx.sghmc(exact_gradient, 3, alpha=0.15, beta=1.0).step(key, q, None, 0.3)


@pytest.mark.parametrize("T", [1.0, 2.0])
def test_sgld_restatement_is_a_correct_sampler(T):
    """Target N(0, 1) per dimension with g = -q: q' = (1 - eps) q + sqrt(2 T eps) z, whose stationary variance is
    exactly 2 T eps / (1 - (1 - eps)^2) = T / (1 - eps / 2).  30 steps from q = 0 at eps = 0.5 (what is left of the
    start: 0.25^30); the pooled variance of the N * D values is within 5 s.e. (5 sqrt(2 / (N D)) = 3.9 %).  A wrong
    noise scale or an ignored temperature misses by 30 % or more."""
    eps = 0.5
    q = np.zeros((N_STAT, D_STAT), f32)
    for k in prng.split(prng.key(31), 30):
        q = rsg.sgld_kernel(k, q, exact_gradient, None, eps, T)
    assert q.dtype == f32
    var, expected = q.astype(np.float64).var(), T / (1.0 - eps / 2.0)
    print("sgld pooled variance", var, "expected", expected, "s.e.", abs(var / expected - 1.0) / SE_REL)
    assert abs(var / expected - 1.0) <= 5.0 * SE_REL


@pytest.mark.parametrize("T", [1.0, 2.0])
def test_sghmc_restatement_is_a_correct_sampler(T):
    """eps = 0.3, alpha = 0.3, beta = 0, L = 5, 12 kernel calls from q = 0 on the same target.  The expected variance
    is the fixed point of the linear recursion of the restated arithmetic (sgmcmc_restatement.sghmc_stationary_variance:
    1.43537 at T = 1, 1.80198 at T = 2, contraction 0.047 per call, so 0.047^12 of the start is left)."""
    eps, alpha, beta, L = 0.3, 0.3, 0.0, 5
    expected, contraction = rsg.sghmc_stationary_variance(eps, alpha, beta, L, T)
    assert abs(expected - {1.0: 1.43537, 2.0: 1.80198}[T]) < 1e-5 and abs(contraction - 0.047) < 1e-3
    q = np.zeros((N_STAT, D_STAT), f32)
    for k in prng.split(prng.key(32), 12):
        q = rsg.sghmc_kernel(k, q, exact_gradient, None, eps, L, T, alpha=alpha, beta=beta)
    var = q.astype(np.float64).var()
    print("sghmc pooled variance", var, "expected", expected, "s.e.", abs(var / expected - 1.0) / SE_REL)
    assert abs(var / expected - 1.0) <= 5.0 * SE_REL


def test_sgnht_restatement_thermostat_holds_the_temperature():
    """eps = 0.05, alpha = 0.1, T = 1 on the same target, 200 steps from q = 0, p = normal, xi = alpha.  The thermostat
    xi' = xi + eps (mean p'^2 - T) is stationary only where E[p^2] = T, so the pooled mean of p^2 is within 5 s.e. of
    T (s.e. of the mean of N * D squared N(0, T) values: T sqrt(2 / (N D))), and xi stays finite."""
    eps, alpha, T = 0.05, 0.1, 1.0
    state = rsg.sgnht_init(np.zeros((N_STAT, D_STAT), f32), prng.key(33), alpha)
    assert state.momentum.shape == (N_STAT, D_STAT) and np.array_equal(state.xi, np.full(N_STAT, alpha, f32))
    for k in prng.split(prng.key(34), 200):
        state = rsg.sgnht_kernel(k, state, exact_gradient, None, eps, T, alpha=alpha)
    assert all(x.dtype == f32 for x in state)
    assert np.isfinite(state.xi).all() and np.isfinite(state.position).all()
    m = (state.momentum.astype(np.float64) ** 2).mean()
    print("sgnht pooled mean p^2", m, "s.e.", abs(m / T - 1.0) / SE_REL, "mean xi", state.xi.mean())
    assert abs(m / T - 1.0) <= 5.0 * SE_REL


def _gaussian_mean_model(prior_sd):
    def logprior_fn(q):
        return -0.5 * (q * q).sum(-1) / prior_sd ** 2

    def loglikelihood_fn(q, minibatch):  # minibatch (B, D) or (N, B, D) -> (N, B)
        y = minibatch if minibatch.ndim == 3 else minibatch[None]
        return -0.5 * ((y - q[:, None, :]) ** 2).sum(-1)

    return logprior_fn, loglikelihood_fn


def test_gradient_helpers_on_cpu_tensors():
    """Gaussian-mean model (prior N(0, s0^2 I), y_b ~ N(q, I)): the autograd estimator equals the closed form
    -q / s0^2 + (M / B) sum_b (y_b - q); control variates with minibatch = data collapse to the full-data gradient."""
    import blackjax_amd as bjx

    N, D, M, B, s0 = 5, 3, 40, 8, 1.5
    rng = np.random.default_rng(0)
    y = (1.0 + rng.standard_normal((M, D))).astype(f32)
    q = rng.standard_normal((N, D)).astype(f32)
    logprior_fn, loglikelihood_fn = _gaussian_mean_model(s0)
    grads = bjx.sgmcmc.gradients
    assert bjx.sgmcmc.grad_estimator is grads.grad_estimator

    est = grads.logdensity_estimator(logprior_fn, loglikelihood_fn, M)
    grad = grads.grad_estimator(logprior_fn, loglikelihood_fn, M)
    r_est, r_grad = rsg.gaussian_mean_logdensity_estimator(s0, M), rsg.gaussian_mean_grad_estimator(s0, M)
    qt, yt = torch.as_tensor(q), torch.as_tensor(y)
    for mb in (y[:B], y[rng.integers(0, M, (N, B))]):  # a shared minibatch, one minibatch per chain
        mbt = torch.as_tensor(mb)
        np.testing.assert_allclose(est(qt, mbt).numpy(), r_est(q, mb), rtol=1e-5)
        g = grad(qt, mbt)
        assert g.shape == (N, D) and g.dtype == torch.float32 and not g.requires_grad and not qt.requires_grad
        closed = -q.astype(np.float64) / s0 ** 2 + (M / B) * (
            (mb if mb.ndim == 3 else mb[None]).astype(np.float64) - q[:, None, :]).sum(1)
        np.testing.assert_allclose(g.numpy(), closed, rtol=1e-5)
        np.testing.assert_allclose(r_grad(q, mb), closed, rtol=1e-6, atol=1e-6)

    for centre in (q[0], q[::-1].copy()):  # (D,) and (N, D)
        calls = []

        def counted(position, minibatch):
            calls.append(minibatch.shape)
            return grad(position, minibatch)

        cv = grads.control_variates(counted, torch.as_tensor(centre), yt)
        assert calls == [yt.shape]  # the full-data gradient at the centre is evaluated once, up front
        np.testing.assert_allclose(cv(qt, yt).numpy(), grad(qt, yt).numpy(), rtol=1e-5)
        r_cv = rsg.control_variates(r_grad, centre, y)
        np.testing.assert_allclose(cv(qt, yt[:B]).numpy(), r_cv(q, y[:B]), rtol=1e-5, atol=1e-4)
        assert len(calls) == 5
