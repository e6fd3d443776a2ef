"""GPU parity of fullrank_vi (blackjax_amd/vi/fullrank_vi.py, csrc/bjx_vi.hip, include/bjx_hip.h "VI") against the
NumPy restatement of the reference's arithmetic, tests/fullrank_vi_restatement.py."""
import numpy as np
import pytest
import torch

import blackjax_amd as bjx
import fullrank_vi_restatement as rv
from blackjax_amd import optim
from blackjax_amd.vi import fullrank_vi as frvi, meanfield_vi as mfvi
from oracle import prng, targets as otargets

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64

T, B = frvi.DRAW_TILE, frvi.COL_BLOCK  # draws per workgroup, columns per block of the triangle
RTOL, ATOL = 1e-6, 1e-7  # test_smc_gpu.py's: fp64 sums rounded once to fp32


def t2n(t):
    return t.detach().cpu().numpy()


def dev_t(a, dev):
    return torch.as_tensor(np.asarray(a), device=dev)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.int32)


def test_tile_and_block_are_the_library_s(dev):
    lib = bjx._lib.load()
    assert lib.bjx_vi_fullrank_tile() == T and lib.bjx_vi_fullrank_block() == B


# ----------------------------------------------------------------------------- sample
# S: one draw, fewer than a thread group's 16, more than a tile.  D: one column, no multiple of 4, one 16-byte piece,
# one less than a block, a block, one more (a second block of one column), two blocks and a rest
@pytest.mark.parametrize("D", [1, 3, 4, B - 1, B, B + 1, 2 * B + 3])
@pytest.mark.parametrize("S", [1, 5, T + 1])
def test_sample_matches_restatement(dev, S, D):
    mu, chol = rv.factor_case(D)
    key = prng.key(100 * S + D)
    ref = rv.sample(key, mu, chol, S)
    state = frvi.FRVIState(dev_t(mu, dev), dev_t(chol, dev), None)
    z = frvi.sample(key, state, S)
    assert z.shape == (S, D) and z.dtype == torch.float32 and z.is_cuda
    np.testing.assert_allclose(t2n(z), ref, rtol=RTOL, atol=ATOL)
    # two calls give identical bits
    assert np.array_equal(bits(t2n(frvi.sample(key, state, S))), bits(t2n(z)))
    # mu four bytes off a 16-byte boundary gives the same bits
    buf = torch.zeros(D + 1, dtype=torch.float32, device=dev)
    buf[1:] = state.mu
    mu_view = buf[1:]
    assert mu_view.data_ptr() % 16 == 4
    z_off = frvi.sample(key, frvi.FRVIState(mu_view, state.chol_params, None), S)
    assert np.array_equal(bits(t2n(z_off)), bits(t2n(z)))
    assert np.array_equal(t2n(state.mu), mu) and np.array_equal(t2n(state.chol_params), chol)
    if S == 1:  # the default is one draw
        assert np.array_equal(bits(t2n(frvi.sample(key, state))), bits(t2n(z)))


# ----------------------------------------------------------------------------- kl_and_grad
def _grad_inputs(S, D):
    """``logp`` and ``G`` as in test_meanfield_vi_gpu.py: random, not a target's values, magnitudes from 1e-2 up to
    1e4, some entries exactly 0."""
    rng = np.random.default_rng(1000 * S + D)
    G = (rng.uniform(-1, 1, (S, D)) * 10.0 ** rng.uniform(-2, 4, (S, D))).astype(f32)
    G[rng.random((S, D)) < 0.1] = 0.0
    logp = (rng.uniform(-1, 1, S) * 10.0 ** rng.uniform(-2, 4, S)).astype(f32)
    logp[rng.random(S) < 0.1] = 0.0
    G.flat[0], G.flat[-1] = 1e4, -1e4
    return logp, G


# S: one row, fewer than a thread group's 16, one less than a tile, a tile, one more, two tiles and a rest (the outer
# product's fills of 32 rows and its chunks split there too).  D: one column, no multiple of 4, one less than a block,
# two blocks with one column in the second, three blocks with a rest
@pytest.mark.parametrize("D", [1, 3, B - 1, B + 1, 2 * B + 3])
@pytest.mark.parametrize("S", [1, 5, T - 1, T, T + 1, 2 * T + 3])
def test_kl_and_grad_matches_restatement(dev, S, D):
    mu, chol = rv.factor_case(D)
    logp, G = _grad_inputs(S, D)
    key = prng.key(7 * S + D)
    mu_g, chol_g, logp_g = dev_t(mu, dev), dev_t(chol, dev), dev_t(logp, dev)
    s_nan, d_nan = S // 2, D // 2
    G_nan = G.copy()
    G_nan[s_nan, d_nan] = np.nan
    keep_mu = np.arange(D) != d_nan
    hit = np.zeros(rv.num_params(D), bool)  # row d_nan of the triangle
    hit[[rv.index(D, d_nan, j) for j in range(d_nan + 1)]] = True
    for stl in (True, False):
        kl_r, g_mu_r, g_chol_r = rv.kl_and_grad(key, mu, chol, logp, G, stl)
        out = frvi.kl_and_grad(key, mu_g, chol_g, logp_g, dev_t(G, dev), stl)
        kl, g_mu, g_chol = out
        assert kl.shape == () and g_mu.shape == (D,) and g_chol.shape == (rv.num_params(D),)
        assert all(o.dtype == torch.float32 and o.is_cuda for o in out)
        np.testing.assert_allclose(t2n(kl), kl_r, rtol=RTOL, atol=ATOL, err_msg=f"kl, stl={stl}")
        np.testing.assert_allclose(t2n(g_mu), g_mu_r, rtol=RTOL, atol=ATOL, err_msg=f"g_mu, stl={stl}")
        np.testing.assert_allclose(t2n(g_chol), g_chol_r, rtol=RTOL, atol=ATOL, err_msg=f"g_chol, stl={stl}")
        # two calls give identical bits
        again = frvi.kl_and_grad(key, mu_g, chol_g, logp_g, dev_t(G, dev), stl)
        for a, b in zip(out, again):
            assert np.array_equal(bits(t2n(a)), bits(t2n(b)))
        # one NaN in G[s, i] reaches g_mu[i] and row i of the triangle, nothing else, and not kl
        kl_n, g_mu_n, g_chol_n = (t2n(o) for o in frvi.kl_and_grad(key, mu_g, chol_g, logp_g, dev_t(G_nan, dev), stl))
        assert np.isnan(g_mu_n[d_nan]) and np.isnan(g_chol_n[hit]).all()
        np.testing.assert_allclose(kl_n, kl_r, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(g_mu_n[keep_mu], g_mu_r[keep_mu], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(g_chol_n[~hit], g_chol_r[~hit], rtol=RTOL, atol=ATOL)
    # the flag changes g_mu and not kl
    a = frvi.kl_and_grad(key, mu_g, chol_g, logp_g, dev_t(G, dev), True)
    b = frvi.kl_and_grad(key, mu_g, chol_g, logp_g, dev_t(G, dev), False)
    assert not torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])


# ----------------------------------------------------------------------------- consistency with meanfield_vi
@pytest.mark.parametrize("S,D", [(5, 3), (T + 1, B + 1)])
def test_zero_strict_lower_triangle_is_meanfield_vi(dev, S, D):
    """With a zero strict lower triangle ``sample``, ``kl``, ``g_mu`` and ``g_chol[:D]`` agree with ``meanfield_vi``'s
    outputs on the device (``rho`` the log-diagonal); the strict-lower gradient is the restatement's, not zero."""
    mu, chol = rv.factor_case(D)
    chol[D:] = 0.0
    logp, G = _grad_inputs(S, D)
    key = prng.key(S + D)
    mu_g, chol_g, rho_g = dev_t(mu, dev), dev_t(chol, dev), dev_t(chol[:D], dev)
    z = frvi.sample(key, frvi.FRVIState(mu_g, chol_g, None), S)
    z_m = mfvi.sample(key, mfvi.MFVIState(mu_g, rho_g, None), S)
    np.testing.assert_allclose(t2n(z), t2n(z_m), rtol=RTOL, atol=ATOL)
    for stl in (True, False):
        kl, g_mu, g_chol = frvi.kl_and_grad(key, mu_g, chol_g, dev_t(logp, dev), dev_t(G, dev), stl)
        kl_m, g_mu_m, g_rho_m = mfvi.kl_and_grad(key, mu_g, rho_g, dev_t(logp, dev), dev_t(G, dev), stl)
        np.testing.assert_allclose(t2n(kl), t2n(kl_m), rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(t2n(g_mu), t2n(g_mu_m), rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(t2n(g_chol[:D]), t2n(g_rho_m), rtol=RTOL, atol=ATOL)
        g_chol_r = rv.kl_and_grad(key, mu, chol, logp, G, stl)[2]
        np.testing.assert_allclose(t2n(g_chol[D:]), g_chol_r[D:], rtol=RTOL, atol=ATOL)
        assert np.abs(g_chol_r[D:]).min() > 0


# ----------------------------------------------------------------------------- argument errors
def test_arguments_are_checked(dev):
    D = 3
    mu, chol = torch.zeros(D, device=dev), torch.zeros(6, device=dev)
    key = prng.key(0)
    state = frvi.init(torch.full((D,), 3.0, device=dev), optim.adam(0.05))
    assert not state.mu.any() and not state.chol_params.any() and state.chol_params.shape == (6,)
    assert torch.equal(frvi.cholesky_factor(state), torch.eye(D, device=dev))
    with pytest.raises(ValueError, match="position must be"):
        frvi.init(torch.zeros(2, 3, device=dev), optim.adam(0.05))
    with pytest.raises(ValueError, match="out of range"):
        frvi.init(torch.zeros(frvi.MAX_DIM + 1, device=dev), optim.adam(0.05))
    with pytest.raises(ValueError, match=r"dim \(dim \+ 1\) / 2 = 6 entries"):
        frvi.sample(key, frvi.FRVIState(mu, torch.zeros(5, device=dev), None))
    with pytest.raises(ValueError, match="must be"):
        frvi.sample(key, frvi.FRVIState(mu, torch.zeros(2, 3, device=dev), None))
    with pytest.raises(TypeError, match="float32"):
        frvi.sample(key, frvi.FRVIState(mu, chol.double(), None))
    with pytest.raises(ValueError, match="num_samples must be at least 1"):
        frvi.sample(key, frvi.FRVIState(mu, chol, None), 0)
    with pytest.raises(ValueError, match="out of range"):
        frvi.sample(key, frvi.FRVIState(mu, chol, None), 2 ** 20 + 1)
    with pytest.raises(ValueError, match="logp and grad must be"):
        frvi.kl_and_grad(key, mu, chol, torch.zeros(4, device=dev), torch.zeros(5, D, device=dev))
    with pytest.raises(ValueError, match="logp and grad must be"):
        frvi.kl_and_grad(key, mu, chol, torch.zeros(4, device=dev), torch.zeros(4, D + 1, device=dev))
    with pytest.raises(ValueError, match=r"parameters\.chol_params must have"):
        frvi.kl_and_grad(key, mu, torch.zeros(7, device=dev), torch.zeros(4, device=dev), torch.zeros(4, D, device=dev))


# ----------------------------------------------------------------------------- full steps
class _Recording:
    """A value-and-gradient callable that keeps the batch it was last called on."""

    _bjx_value_and_grad = True
    _bjx_returns_pair = True

    def __init__(self, target):
        self.target, self.z = target, None

    def __call__(self, q):
        self.z = q.clone()
        return self.target(q)


def _plain_ar1(rho, D, dev, mean=None):
    """The AR(1) Gaussian as a plain PyTorch function of the batch: the tridiagonal quadratic form."""
    c = 1.0 / (1.0 - rho * rho)
    diag = torch.full((D,), (1.0 + rho * rho) * c, device=dev)
    diag[0] = diag[-1] = c
    off = rho * c

    def fn(z):
        d = z if mean is None else z - mean
        quad = (diag * d * d).sum(-1)
        if D > 1:
            quad = quad - 2.0 * off * (d[:, 1:] * d[:, :-1]).sum(-1)
        return -0.5 * quad

    return fn


def _resync(state):
    """The device's state as the restatement's."""
    o = state.opt_state
    return rv.FRVIState(t2n(state.mu), t2n(state.chol_params),
                        rv.AdamState(o.count, tuple(t2n(m) for m in o.mu), tuple(t2n(v) for v in o.nu)))


@pytest.mark.parametrize("S,D", list(rv.FULL_CASES))
def test_steps_match_restatement(dev, S, D):
    """Four steps with ``adam(0.05)`` on the AR(1) Gaussian, as a ``targets.AR1Gaussian`` and as a plain PyTorch
    function, the restatement re-synchronised to the device's state before every step: ``mu``, ``chol_params`` and the
    optimiser's moments at the standing tolerances.  No coordinate is left out: the keys keep every gradient of the
    restatement above 1e-4 (test_fullrank_vi_api.py)."""
    keys = rv.full_case(S, D)
    fn_r = otargets.ar1_gaussian(rv.FULL_RHO, D)
    recording = _Recording(bjx.targets.AR1Gaussian(rv.FULL_RHO, D))
    for name, fn_g in (("AR1Gaussian", recording), ("plain", _plain_ar1(rv.FULL_RHO, D, dev))):
        opt_g, opt_r = optim.adam(rv.FULL_LR), rv.Adam(rv.FULL_LR)
        state = frvi.init(torch.full((D,), 3.0, device=dev), opt_g)
        assert state.opt_state.count == 0 and isinstance(state.opt_state.mu, tuple) and len(state.opt_state.mu) == 2
        for t, k in enumerate(keys):
            state_r, kl_r = rv.step(k, _resync(state), fn_r, opt_r, S)
            drawn = frvi.sample(k, state, S)
            new, info = frvi.step(k, state, fn_g, opt_g, S)
            assert isinstance(new, frvi.FRVIState) and isinstance(info, frvi.FRVIInfo)
            assert info.elbo.shape == () and info.elbo.is_cuda and new.opt_state.count == t + 1
            msg = f"{name}, step {t}"
            np.testing.assert_allclose(t2n(new.mu), state_r.mu, rtol=RTOL, atol=ATOL, err_msg=msg)
            np.testing.assert_allclose(t2n(new.chol_params), state_r.chol_params, rtol=RTOL, atol=ATOL, err_msg=msg)
            for got, want in zip(new.opt_state.mu + new.opt_state.nu, state_r.opt_state.mu + state_r.opt_state.nu):
                np.testing.assert_allclose(t2n(got), want, rtol=RTOL, atol=ATOL, err_msg=msg)
            if fn_g is recording:
                # step uses the key as sample does, and with the target's own kernel logp is the restatement's
                assert torch.equal(recording.z, drawn)
                np.testing.assert_allclose(t2n(info.elbo), kl_r, rtol=RTOL, atol=ATOL, err_msg=msg)
            state = new


def test_other_optimisers_and_the_top_level_api(dev):
    """Any object with ``init`` / ``update`` that takes tensors works: the step only adds the updates it returns.  The
    top-level API draws 100 points per step."""
    D = 3
    recording = _Recording(bjx.targets.AR1Gaussian(0.9, D))

    class Descent:
        def init(self, params):
            return 0

        def update(self, grads, state, params=None):
            return tuple(-0.1 * g for g in grads), state + 1

    alg = bjx.fullrank_vi(recording, Descent())
    state = alg.init(torch.zeros(D, device=dev))
    key = prng.key(3)
    new, info = alg.step(key, state)
    assert recording.z.shape == (100, D) and new.opt_state == 1
    kl, g_mu, g_chol = frvi.kl_and_grad(key, state.mu, state.chol_params, *recording.target(recording.z))
    assert torch.equal(new.mu, state.mu + -0.1 * g_mu)
    assert torch.equal(new.chol_params, state.chol_params + -0.1 * g_chol)
    assert torch.equal(info.elbo, kl)
    assert alg.sample(key, new).shape == (1, D) and alg.sample(key, new, 7).shape == (7, D)
    # sgd from the package
    new, _ = frvi.step(key, frvi.init(torch.zeros(D, device=dev), optim.sgd(0.1)), recording, optim.sgd(0.1), 100)
    np.testing.assert_allclose(t2n(new.mu), t2n(-0.1 * g_mu), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(t2n(new.chol_params), t2n(-0.1 * g_chol), rtol=RTOL, atol=ATOL)


# ----------------------------------------------------------------------------- no host read
def test_a_step_reads_nothing_back(dev):
    """After a first step (which traces the function and compiles what it needs) two steps and a draw under
    ``torch.cuda.set_sync_debug_mode("error")`` raise nothing."""
    D = rv.CONV_D
    m = dev_t(rv.CONV_M, dev)
    algs = [bjx.fullrank_vi(_plain_ar1(rv.CONV_RHO, D, dev, m), optim.adam(0.05), num_samples=32),
            bjx.fullrank_vi(bjx.targets.AR1Gaussian(rv.CONV_RHO, D), optim.sgd(0.01), num_samples=32)]
    keys = prng.split(prng.key(9), 4)
    states = [alg.step(keys[0], alg.init(torch.zeros(D, device=dev)))[0] for alg in algs]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i, alg in enumerate(algs):
            for k in keys[1:3]:
                states[i], info = alg.step(k, states[i])
            z = alg.sample(keys[3], states[i], 8)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert z.shape == (8, D) and bool(torch.isfinite(info.elbo))
    assert states[0].opt_state.count == 3 and all(bool(torch.isfinite(st.mu).all()) for st in states)


# ----------------------------------------------------------------------------- end to end
def test_converges_on_the_correlated_gaussian(dev):
    """The convergence case of test_fullrank_vi_api.py on the device, the target a plain PyTorch function: with STL the
    run ends inside the restatement's bounds (ten times its own worst of five keys, 9.54e-7 for ``mu`` and 1.23e-6 for
    ``L L^T``: a floor of fp32 rounding noise), without STL it stays more than 1e-2 from the mean.
    ``cholesky_factor(state)`` times its transpose is the target's covariance within that bound.  A ``meanfield_vi`` fit
    of the same target with the same keys ends with variances ``exp(2 rho)`` below half the true marginal variances
    (its optimum is ``1 / diag(C^-1)``): the case full-rank VI exists for."""
    D = rv.CONV_D
    fn = _plain_ar1(rv.CONV_RHO, D, dev, dev_t(rv.CONV_M, dev))
    opt = optim.adam(rv.CONV_LR)
    keys = prng.split(prng.key(rv.CONV_SEEDS[0]), rv.CONV_STEPS)
    alg = bjx.fullrank_vi(fn, opt, num_samples=rv.CONV_S)
    state = alg.init(torch.zeros(D, device=dev))
    for k in keys:
        state, info = alg.step(k, state)
    err_mu, err_cov = rv.conv_errors(t2n(state.mu), t2n(state.chol_params))
    print("device, STL:", err_mu, err_cov, "kl", float(info.elbo))
    assert err_mu <= rv.CONV_MU_BOUND and err_cov <= rv.CONV_COV_BOUND
    L = frvi.cholesky_factor(state)
    assert L.shape == (D, D) and bool((L.triu(1) == 0).all())
    cov = t2n(L.double() @ L.double().T)
    assert np.max(np.abs(cov - otargets.ar1_covariance(rv.CONV_RHO, D))) <= rv.CONV_COV_BOUND

    free = frvi.init(torch.zeros(D, device=dev), opt)
    for k in keys:
        free, _ = frvi.step(k, free, fn, opt, rv.CONV_S, stl_estimator=False)
    err_free, _ = rv.conv_errors(t2n(free.mu), t2n(free.chol_params))
    print("device, no STL:", err_free)
    assert err_free > 1e-2

    mf = bjx.meanfield_vi(fn, opt, num_samples=rv.CONV_S)
    mstate = mf.init(torch.zeros(D, device=dev))
    for k in keys:
        mstate, _ = mf.step(k, mstate)
    var = np.exp(2.0 * t2n(mstate.rho).astype(f64))
    true_var = np.diag(otargets.ar1_covariance(rv.CONV_RHO, D)).astype(f64)
    print("meanfield variances over the true ones:", var / true_var)
    assert (var < 0.5 * true_var).all()
