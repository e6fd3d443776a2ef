"""API surface of meanfield_vi (blackjax_amd/vi/meanfield_vi.py, include/bjx_hip.h "VI") and the arithmetic of its
NumPy restatement, tests/meanfield_vi_restatement.py.  Needs no GPU."""
import inspect

import numpy as np
import pytest
import torch

import blackjax_amd as bjx
import meanfield_vi_restatement as rv
from blackjax_amd import _lib, optim
from blackjax_amd.vi import meanfield_vi as mfvi
from oracle import prng, targets as otargets

f32, f64 = np.float32, np.float64


def _defaults(fn):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty}


# ----------------------------------------------------------------------------- names and signatures
def test_names_and_signatures():
    for name in ("meanfield_vi", "vi", "VIAlgorithm"):
        assert name in bjx.__all__ and hasattr(bjx, name)
    assert inspect.ismodule(bjx.vi) and "meanfield_vi" in bjx.vi.__all__ and bjx.vi.meanfield_vi is mfvi
    assert bjx.VIAlgorithm._fields == ("init", "step", "sample")
    assert isinstance(bjx.meanfield_vi, bjx.GenerateVariationalAPI)
    assert bjx.meanfield_vi.init is mfvi.init and bjx.meanfield_vi.step is mfvi.step
    assert bjx.meanfield_vi.sample is mfvi.sample
    for name in ("MFVIState", "MFVIInfo", "init", "step", "sample", "kl_and_grad", "generate_meanfield_logdensity",
                 "as_top_level_api"):
        assert name in mfvi.__all__ and hasattr(mfvi, name)
    assert mfvi.MFVIState._fields == ("mu", "rho", "opt_state") and mfvi.MFVIInfo._fields == ("elbo",)
    assert list(inspect.signature(mfvi.init).parameters) == ["position", "optimizer"]
    assert list(inspect.signature(mfvi.step).parameters) == ["rng_key", "state", "logdensity_fn", "optimizer",
                                                             "num_samples", "stl_estimator"]
    assert _defaults(mfvi.step) == {"num_samples": 5, "stl_estimator": True}
    assert list(inspect.signature(mfvi.sample).parameters) == ["rng_key", "state", "num_samples"]
    assert _defaults(mfvi.sample) == {"num_samples": 1}
    assert list(inspect.signature(mfvi.kl_and_grad).parameters) == ["rng_key", "mu", "rho", "logp", "grad",
                                                                    "stl_estimator"]
    assert _defaults(mfvi.kl_and_grad) == {"stl_estimator": True}
    assert list(inspect.signature(mfvi.generate_meanfield_logdensity).parameters) == ["mu", "rho"]
    assert list(inspect.signature(mfvi.as_top_level_api).parameters) == ["logdensity_fn", "optimizer", "num_samples"]
    assert _defaults(mfvi.as_top_level_api) == {"num_samples": 100}
    alg = bjx.meanfield_vi(lambda z: -(z * z).sum(-1), optim.adam(0.05))
    assert isinstance(alg, bjx.VIAlgorithm)
    assert list(inspect.signature(alg.init).parameters) == ["position"]
    assert list(inspect.signature(alg.step).parameters) == ["rng_key", "state"]
    assert list(inspect.signature(alg.sample).parameters) == ["rng_key", "state", "num_samples"]
    assert _defaults(alg.sample) == {"num_samples": 1}


def test_host_tensors_are_refused():
    """There is no CPU fallback: parameters on the host raise before anything is launched."""
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mfvi.init(torch.zeros(3), optim.adam(0.05))
    state = mfvi.MFVIState(torch.zeros(3), torch.zeros(3), None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mfvi.sample(prng.key(0), state, 2)


def test_entry_points_check_their_arguments():
    lib = _lib.load()
    assert lib.bjx_vi_meanfield_tile() == mfvi.GRAD_TILE
    T = mfvi.GRAD_TILE
    for S, D in ((1, 1), (T, 256), (T + 1, 257), (5, 300000)):
        tiles, blocks = -(-S // T), -(-D // 256)
        assert lib.bjx_vi_meanfield_grad_workspace_bytes(S, D) == 8 * (3 * tiles * D + 2 * blocks)
    for S, D in ((0, 4), (4, 0), (2 ** 24 + 1, 1), (1, 2 ** 20 + 1), (2 ** 12, 2 ** 20)):
        assert lib.bjx_vi_meanfield_grad_workspace_bytes(S, D) == 0
        assert lib.bjx_vi_meanfield_sample(None, 1, 2, S, D, None, None, None) != 0
        assert b"bjx_vi_meanfield_sample: bad sizes" in lib.bjx_last_error()
        assert lib.bjx_vi_meanfield_grad(None, 1, 2, S, D, 1, None, None, None, None, None, None, None) != 0
        assert b"bjx_vi_meanfield_grad: bad sizes" in lib.bjx_last_error()
    assert lib.bjx_vi_meanfield_grad(None, 1, 2, 4, 4, 2, None, None, None, None, None, None, None) != 0
    assert lib.bjx_vi_meanfield_sample(None, 1, 2, 4, 4, None, None, None) != 0
    assert b"bjx_vi_meanfield_sample: null pointer" in lib.bjx_last_error()
    assert lib.bjx_vi_meanfield_grad(None, 1, 2, 4, 4, 0, None, None, None, None, None, None, None) != 0
    assert b"bjx_vi_meanfield_grad: null pointer" in lib.bjx_last_error()
    assert lib.bjx_optim_adam(None, -1, *([0.5] * 9), *([None] * 6)) != 0
    assert b"bjx_optim_adam: bad sizes" in lib.bjx_last_error()
    assert lib.bjx_optim_adam(None, 4, *([0.5] * 9), *([None] * 6)) != 0
    assert b"bjx_optim_adam: null pointer" in lib.bjx_last_error()
    assert lib.bjx_optim_sgd(None, 4, 0.5, None, None) != 0 and b"bjx_optim_sgd: null pointer" in lib.bjx_last_error()
    assert lib.bjx_optim_adam(None, 0, *([0.5] * 9), *([None] * 6)) == 0  # nothing to do
    assert lib.bjx_optim_sgd(None, 0, 0.5, None, None) == 0


# ----------------------------------------------------------------------------- the formulas against autograd
@pytest.mark.parametrize("stl", [True, False])
@pytest.mark.parametrize("S,D", [(5, 3), (7, 4)])
def test_gradient_formulas_match_autograd_of_the_reference_lines(S, D, stl):
    """The restatement's gradient formulas against ``torch.autograd`` in fp64 of the reference's literal lines:
    ``z = mu + exp(rho) * eps``, ``logq`` the sum of the normal log-pdfs of ``z`` with ``(mu, rho)`` detached under
    STL, ``kl = (logq - logp).mean()``.  The target is a non-Gaussian function, so that ``G`` depends on ``z``."""
    rng = np.random.default_rng(10 * S + D)
    eps = torch.as_tensor(prng.normal(prng.key(S + D), (S, D)).astype(f64))
    mu = torch.as_tensor(rng.standard_normal(D), dtype=torch.float64).requires_grad_(True)
    rho = torch.as_tensor(rng.uniform(-1.5, 0.5, D), dtype=torch.float64).requires_grad_(True)
    a, b = torch.as_tensor(rng.standard_normal(D)), torch.as_tensor(rng.uniform(0.5, 2.0, D))

    def logp_fn(z):
        return (-0.5 * b * (z - a) ** 2 + torch.sin(z)).sum(-1) + 0.1 * z.prod(-1)

    z = mu + torch.exp(rho) * eps
    mu_q, rho_q = (mu.detach(), rho.detach()) if stl else (mu, rho)
    logq = torch.distributions.Normal(mu_q, torch.exp(rho_q)).log_prob(z).sum(-1)
    kl = (logq - logp_fn(z)).mean()
    g_mu, g_rho = torch.autograd.grad(kl, (mu, rho))

    zd = z.detach().requires_grad_(True)
    logp = logp_fn(zd)
    (G,) = torch.autograd.grad(logp.sum(), zd)
    kl_r, g_mu_r, g_rho_r = rv.kl_and_grad_terms(eps.numpy(), np.exp(rho.detach().numpy()), rho.detach().numpy(),
                                                 logp.detach().numpy(), G.numpy(), stl)
    np.testing.assert_allclose(kl_r, kl.item(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(g_mu_r, g_mu.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(g_rho_r, g_rho.numpy(), rtol=1e-12, atol=1e-12)
    # the approximation's log-density, restated and as the package forms it
    np.testing.assert_allclose(rv.meanfield_logdensity(mu.detach().numpy(), rho.detach().numpy(), z.detach().numpy()),
                               logq.detach().numpy(), rtol=1e-12, atol=1e-12)
    ld = mfvi.generate_meanfield_logdensity(mu.detach(), rho.detach())(z.detach())
    assert ld.shape == (S,)
    np.testing.assert_allclose(ld.numpy(), logq.detach().numpy(), rtol=1e-12, atol=1e-12)


def test_restated_sample_and_step_are_consistent():
    """``sample`` is one fused multiply-add on the draws of the key itself; ``step`` draws what ``sample`` returns and
    applies the restated Adam to the rounded gradients."""
    S, D = 7, 4
    key = prng.key(5)
    mu, rho = np.linspace(-1, 1, D).astype(f32), np.linspace(-2, 0.5, D).astype(f32)
    z = rv.sample(key, mu, rho, S)
    eps = prng.normal(key, (S, D))
    sigma = np.exp(rho.astype(f64)).astype(f32)
    assert z.dtype == f32 and z.shape == (S, D)
    assert np.array_equal(z, (sigma.astype(f64) * eps.astype(f64) + mu.astype(f64)).astype(f32))  # exact product: 48 bits
    opt = rv.Adam(0.05)
    state = rv.MFVIState(mu, rho, opt.init((mu, rho)))
    fn = otargets.diag_gaussian(np.linspace(0.5, 2.0, D).astype(f32))
    new, kl = rv.step(key, state, fn, opt, S)
    logp, G = fn(z)
    kl_r, g_mu, g_rho = rv.kl_and_grad(key, mu, rho, logp, G)
    u, opt_state = opt.update((g_mu.astype(f32), g_rho.astype(f32)), state.opt_state)
    assert kl == f32(kl_r) and new.opt_state.count == 1
    assert np.array_equal(new.mu, mu + u[0]) and np.array_equal(new.rho, rho + u[1])
    # kl as the issue writes it for the kernel: no per-row pass
    kl_flat = (-(eps.astype(f64) ** 2).sum() / (2 * S) - rho.astype(f64).sum() - D * rv.LOG_2PI / 2
               - logp.astype(f64).mean())
    np.testing.assert_allclose(kl_r, kl_flat, rtol=1e-13)


# ----------------------------------------------------------------------------- the optimisers
_GRADS = (0.5, -1.25, 3e-3, 0.0, 1e-20)
# (update, mu, nu) bit patterns of optim.adam on one host scalar, step after step over _GRADS, recorded from the code
# as it stood before the device path was added
_ADAM_BITS = {
    (0.05,): [(0xbd4ccc73, 0x3d4ccccd, 0x3983126f), (0x3cb5212a, 0xbda3d70a, 0x3aed8905),
              (0x3c8b6e4b, 0xbd92d773, 0x3aed4c83), (0x3c646cd3, 0xbd84284e, 0x3aed0fc4),
              (0x3c411249, 0xbd6de226, 0x3aecd314)],
    (0.01, 0.8, 0.99, 1e-06, 0.001): [(0xbc23834e, 0x3dcccccd, 0x3b23d70a), (0x3ba228ff, 0xbe2e147a, 0x3c944674),
                                      (0x3b69e898, 0xbe0aa64c, 0x3c92cb0e), (0x3b330021, 0xbdddd6e0, 0x3c915344),
                                      (0x3b0ce944, 0xbdb178b3, 0x3c8fdf3c)],
}
_SGD_BITS = [0xbd4ccccd, 0x3e000000, 0xb99d4952, 0x80000000, 0x9c971da0]  # optim.sgd(0.1) over _GRADS


def _u32(x):
    return int(np.asarray(x, f32).view(np.uint32))


def test_host_scalar_optimisers_are_unchanged():
    for args, expected in _ADAM_BITS.items():
        opt = optim.adam(*args)
        state = opt.init(0.0)
        assert state == optim.ScaleByAdamState(0, f32(0.0), f32(0.0))
        for t, (g, bits) in enumerate(zip(_GRADS, expected)):
            u, state = opt.update(g, state, 0.0)
            assert isinstance(u, np.float32) and isinstance(state.mu, np.float32) and state.count == t + 1
            assert (_u32(u), _u32(state.mu), _u32(state.nu)) == bits, (args, t)
    sgd = optim.sgd(0.1)
    assert sgd.init(0.0) == ()
    for g, bits in zip(_GRADS, _SGD_BITS):
        u, state = sgd.update(g, ())
        assert isinstance(u, np.float32) and _u32(u) == bits and state == ()


def test_restated_optimisers_are_the_scalar_code_element_by_element():
    rng = np.random.default_rng(3)
    grads = [(rng.standard_normal(5) * 10.0 ** rng.integers(-6, 4, 5)).astype(f32) for _ in range(3)]
    for args in _ADAM_BITS:
        vec, sca = rv.Adam(*args), optim.adam(*args)
        st_v, st_s = vec.init((grads[0],)), [sca.init(0.0) for _ in range(5)]
        for g in grads:
            (u,), st_v = vec.update((g,), st_v)
            outs = [sca.update(g[i], st_s[i]) for i in range(5)]
            st_s = [o[1] for o in outs]
            assert np.array_equal(u.view(np.int32), np.array([o[0] for o in outs], f32).view(np.int32))
            assert np.array_equal(st_v.mu[0], np.array([s.mu for s in st_s], f32))
            assert np.array_equal(st_v.nu[0], np.array([s.nu for s in st_s], f32))
    (u,), _ = rv.SGD(0.1).update((grads[0],), ())
    assert np.array_equal(u, np.array([optim.sgd(0.1).update(g, ())[0] for g in grads[0]], f32))


# ----------------------------------------------------------------------------- the full-step keys, convergence
def test_full_step_keys_keep_every_gradient_away_from_zero():
    """The keys of test_meanfield_vi_gpu.py's full-step cases: in the restatement no coordinate of either gradient is
    below 1e-4 in magnitude at any of the four steps, so no coordinate is left out of that comparison."""
    for (S, D) in rv.FULL_CASES:
        inv_var, keys = rv.full_case(S, D)
        fn, opt = otargets.diag_gaussian(inv_var), rv.Adam(rv.FULL_LR)
        state = rv.init(np.zeros(D, f32), opt)
        for k in keys:
            logp, G = fn(rv.sample(k, state.mu, state.rho, S))
            _, g_mu, g_rho = rv.kl_and_grad(k, state.mu, state.rho, logp, G)
            assert min(np.abs(g_mu).min(), np.abs(g_rho).min()) >= 1e-4, (S, D)
            state, _ = rv.step(k, state, fn, opt, S)


def test_restated_sampler_converges_on_the_diagonal_gaussian():
    """The convergence case (D = 16, S = 32, adam(0.05), 600 steps) in the restatement.  With STL the estimator's
    variance vanishes at the optimum and the run ends at the rounding floor recorded above; without STL the same run
    stays more than 1e-2 from the mean, which shows the flag to act.  The restatement's own worst over the five keys
    of ``CONV_SEEDS``, with the project's draws and STL on, was max|mu - m| = 2.62e-6 and max|rho - log s| = 9.06e-8;
    without STL the five runs ended 0.117 to 0.217 from m."""
    seed = rv.CONV_SEEDS[0]
    err_mu, err_rho, _ = rv.converge(seed, True)
    print("restatement, STL:", err_mu, err_rho)
    assert err_mu <= rv.CONV_MU_BOUND and err_rho <= rv.CONV_RHO_BOUND
    err_mu, err_rho, _ = rv.converge(seed, False)
    print("restatement, no STL:", err_mu, err_rho)
    assert err_mu > 1e-2
