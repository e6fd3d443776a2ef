"""GPU parity of meanfield_vi (blackjax_amd/vi/meanfield_vi.py, csrc/bjx_vi.hip, include/bjx_hip.h "VI") and of the
device path of blackjax_amd/optim.py against the NumPy restatement of the reference's arithmetic,
tests/meanfield_vi_restatement.py."""
import numpy as np
import pytest
import torch

import blackjax_amd as bjx
import meanfield_vi_restatement as rv
from blackjax_amd import optim
from blackjax_amd.vi import meanfield_vi as mfvi
from oracle import prng, targets as otargets

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64

T = mfvi.GRAD_TILE  # rows per workgroup of the reduction
RTOL, ATOL = 1e-6, 1e-7  # test_smc_gpu.py's: fp64 sums rounded once to fp32


def t2n(t):
    return t.detach().cpu().numpy()


def dev_t(a, dev):
    return torch.as_tensor(np.asarray(a), device=dev)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.int32)


def _parameters(d):
    rng = np.random.default_rng(d)
    return rng.standard_normal(d).astype(f32), rng.uniform(-2.5, 1.0, d).astype(f32)


# ----------------------------------------------------------------------------- sample
# one element; 4-byte sweeps; one 16-byte piece per row; an odd row length over more than one wavefront; 16-byte pieces
# over more than one workgroup; more rows than the reduction's tile
@pytest.mark.parametrize("S,D", [(1, 1), (5, 3), (7, 4), (5, 65), (3, 260), (T + 1, 4)])
def test_sample_is_bit_exact(dev, S, D):
    mu, rho = _parameters(D)
    key = prng.key(100 * S + D)
    ref = rv.sample(key, mu, rho, S)
    state = mfvi.MFVIState(dev_t(mu, dev), dev_t(rho, dev), None)
    z = mfvi.sample(key, state, S)
    assert z.shape == (S, D) and z.dtype == torch.float32 and z.is_cuda
    assert np.array_equal(bits(t2n(z)), bits(ref))
    # mu four bytes off a 16-byte boundary: the 4-byte sweeps whatever D is
    buf = torch.zeros(D + 1, dtype=torch.float32, device=dev)
    buf[1:] = state.mu
    mu_view = buf[1:]
    assert mu_view.data_ptr() % 16 == 4
    z = mfvi.sample(key, mfvi.MFVIState(mu_view, state.rho, None), S)
    assert np.array_equal(bits(t2n(z)), bits(ref))
    assert np.array_equal(t2n(state.mu), mu) and np.array_equal(t2n(state.rho), rho)
    if S == 1:  # the default is one draw
        assert np.array_equal(bits(t2n(mfvi.sample(key, state))), bits(ref))


# ----------------------------------------------------------------------------- kl_and_grad
def _grad_inputs(S, D):
    """Random ``logp`` and ``G``, not a target's values: magnitudes from 1e-2 up to 1e4, some entries exactly 0."""
    rng = np.random.default_rng(1000 * S + D)
    G = (rng.uniform(-1, 1, (S, D)) * 10.0 ** rng.uniform(-2, 4, (S, D))).astype(f32)
    G[rng.random((S, D)) < 0.1] = 0.0
    logp = (rng.uniform(-1, 1, S) * 10.0 ** rng.uniform(-2, 4, S)).astype(f32)
    logp[rng.random(S) < 0.1] = 0.0
    G.flat[0], G.flat[-1] = 1e4, -1e4
    mu, rho = _parameters(D)
    return mu, rho, logp, G


# S: one row, fewer than a column's row groups, one less than a tile, a tile, one more, two tiles and a rest.
# D: one column, no multiple of 4, the 4-column block, the 16- and 64-column blocks with a partial last block
@pytest.mark.parametrize("D", [1, 3, 4, 65, 260])
@pytest.mark.parametrize("S", [1, 5, T - 1, T, T + 1, 2 * T + 3])
def test_kl_and_grad_matches_restatement(dev, S, D):
    mu, rho, logp, G = _grad_inputs(S, D)
    key = prng.key(7 * S + D)
    mu_g, rho_g, logp_g = dev_t(mu, dev), dev_t(rho, dev), dev_t(logp, dev)
    s_nan, d_nan = S // 2, D // 2
    G_nan = G.copy()
    G_nan[s_nan, d_nan] = np.nan
    keep = np.arange(D) != d_nan
    for stl in (True, False):
        kl_r, g_mu_r, g_rho_r = rv.kl_and_grad(key, mu, rho, logp, G, stl)
        out = mfvi.kl_and_grad(key, mu_g, rho_g, logp_g, dev_t(G, dev), stl)
        kl, g_mu, g_rho = out
        assert kl.shape == () and g_mu.shape == (D,) and g_rho.shape == (D,)
        assert all(o.dtype == torch.float32 and o.is_cuda for o in out)
        np.testing.assert_allclose(t2n(kl), kl_r, rtol=RTOL, atol=ATOL, err_msg=f"kl, stl={stl}")
        np.testing.assert_allclose(t2n(g_mu), g_mu_r, rtol=RTOL, atol=ATOL, err_msg=f"g_mu, stl={stl}")
        np.testing.assert_allclose(t2n(g_rho), g_rho_r, rtol=RTOL, atol=ATOL, err_msg=f"g_rho, stl={stl}")
        # two calls give identical bits
        again = mfvi.kl_and_grad(key, mu_g, rho_g, logp_g, dev_t(G, dev), stl)
        for a, b in zip(out, again):
            assert np.array_equal(bits(t2n(a)), bits(t2n(b)))
        # one NaN in G poisons its own column of both gradients and nothing else
        kl_n, g_mu_n, g_rho_n = (t2n(o) for o in mfvi.kl_and_grad(key, mu_g, rho_g, logp_g, dev_t(G_nan, dev), stl))
        assert np.isnan(g_mu_n[d_nan]) and np.isnan(g_rho_n[d_nan])
        np.testing.assert_allclose(kl_n, kl_r, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(g_mu_n[keep], g_mu_r[keep], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(g_rho_n[keep], g_rho_r[keep], rtol=RTOL, atol=ATOL)
    if S > 1:  # the flag acts
        a = mfvi.kl_and_grad(key, mu_g, rho_g, logp_g, dev_t(G, dev), True)
        b = mfvi.kl_and_grad(key, mu_g, rho_g, logp_g, dev_t(G, dev), False)
        assert not torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])


# ----------------------------------------------------------------------------- the device optimisers
def _optim_grads(n, steps=3):
    rng = np.random.default_rng(n)
    gs = [(rng.standard_normal(n) * 10.0 ** rng.integers(-8, 6, n)).astype(f32) for _ in range(steps)]
    gs[1][rng.random(n) < 0.2] = 0.0
    return gs


# one element, 4-byte and 16-byte sizes, a partial second wavefront, more than one workgroup
@pytest.mark.parametrize("n", [1, 3, 4, 65, 1025])
def test_device_optimisers_are_the_scalar_code_bit_for_bit(dev, n):
    """Three successive ``adam`` updates, and ``sgd``, on (n,) device tensors against the scalar code of optim.py applied
    element by element on the host: the existing code is the reference."""
    grads = _optim_grads(n)
    for args in ((0.05,), (0.01, 0.8, 0.99, 1e-6, 1e-3)):
        opt = optim.adam(*args)
        p = torch.zeros(n, device=dev)
        state = opt.init(p)
        assert state.count == 0 and state.mu.shape == (n,) and state.mu.is_cuda and not state.mu.any()
        host = [opt.init(0.0) for _ in range(n)]
        for t, g in enumerate(grads):
            g_g = dev_t(g, dev)
            u, new = opt.update(g_g, state, p)
            assert isinstance(new.count, int) and new.count == t + 1
            assert new.mu.data_ptr() != state.mu.data_ptr() and np.array_equal(t2n(g_g), g)  # out of place
            outs = [opt.update(g[i], host[i]) for i in range(n)]
            host = [o[1] for o in outs]
            assert np.array_equal(bits(t2n(u)), bits([o[0] for o in outs])), (args, t)
            assert np.array_equal(bits(t2n(new.mu)), bits([s.mu for s in host])), (args, t)
            assert np.array_equal(bits(t2n(new.nu)), bits([s.nu for s in host])), (args, t)
            state = new
    # a tuple of tensors: the state has its structure, one count for all leaves
    opt = optim.adam(0.05)
    pair = (torch.zeros(n, device=dev), torch.zeros(3, device=dev))
    state = opt.init(pair)
    assert isinstance(state.mu, tuple) and [m.shape for m in state.mu] == [(n,), (3,)]
    g3 = np.array([0.5, -1.25, 3e-3], f32)
    (u0, u1), state = opt.update((dev_t(grads[0], dev), dev_t(g3, dev)), state, pair)
    assert state.count == 1 and isinstance(state.nu, tuple)
    single = opt.update(dev_t(grads[0], dev), opt.init(pair[0]))[0]
    assert torch.equal(u0, single)
    assert np.array_equal(bits(t2n(u1)), bits([opt.update(g, opt.init(0.0))[0] for g in g3]))
    # sgd
    sgd = optim.sgd(0.1)
    assert sgd.init(pair) == ()
    u, st = sgd.update(dev_t(grads[0], dev), ())
    assert st == () and np.array_equal(bits(t2n(u)), bits([sgd.update(g, ())[0] for g in grads[0]]))
    (u0, u1), _ = sgd.update((dev_t(grads[0], dev), dev_t(g3, dev)), ())
    assert torch.equal(u0, u) and np.array_equal(bits(t2n(u1)), bits([sgd.update(g, ())[0] for g in g3]))


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


def _resync(state):
    """The device's state as the restatement's."""
    o = state.opt_state
    return rv.MFVIState(t2n(state.mu), t2n(state.rho),
                        rv.AdamState(o.count, tuple(t2n(m) for m in o.mu), tuple(t2n(v) for v in o.nu)))


@pytest.mark.parametrize("S,D", list(rv.FULL_CASES))
def test_steps_match_restatement(dev, S, D):
    """Four steps with ``adam(0.05)`` on a zero-mean diagonal Gaussian, as a ``targets.DiagGaussian`` and as a plain
    PyTorch function (traced into one kernel), the restatement re-synchronised to the device's state before every
    step: ``mu``, ``rho`` and the optimiser's moments at the standing tolerances.  No coordinate is left out: the keys
    keep every gradient of the restatement above 1e-4 (test_meanfield_vi_api.py)."""
    inv_var, keys = rv.full_case(S, D)
    iv_g = dev_t(inv_var, dev)
    fn_r = otargets.diag_gaussian(inv_var)
    recording = _Recording(bjx.targets.DiagGaussian(iv_g))

    def plain(z):
        return (-0.5 * z * z * iv_g).sum(-1)

    for name, fn_g in (("DiagGaussian", recording), ("plain", plain)):
        opt_g, opt_r = optim.adam(rv.FULL_LR), rv.Adam(rv.FULL_LR)
        state = mfvi.init(torch.full((D,), 3.0, device=dev), opt_g)
        assert not state.mu.any() and bool((state.rho == -2.0).all()) and state.opt_state.count == 0
        assert isinstance(state.opt_state.mu, tuple) and len(state.opt_state.mu) == 2
        for t, k in enumerate(keys):
            state_r, kl_r = rv.step(k, _resync(state), fn_r, opt_r, S)
            drawn = mfvi.sample(k, state, S)
            new, info = mfvi.step(k, state, fn_g, opt_g, S)
            assert isinstance(new, mfvi.MFVIState) and isinstance(info, mfvi.MFVIInfo)
            assert info.elbo.shape == () and info.elbo.is_cuda and new.opt_state.count == t + 1
            msg = f"{name}, step {t}"
            np.testing.assert_allclose(t2n(new.mu), state_r.mu, rtol=RTOL, atol=ATOL, err_msg=msg)
            np.testing.assert_allclose(t2n(new.rho), state_r.rho, rtol=RTOL, atol=ATOL, err_msg=msg)
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
    iv_g = dev_t(np.linspace(0.5, 2.0, D).astype(f32), dev)
    recording = _Recording(bjx.targets.DiagGaussian(iv_g))

    class Descent:
        def init(self, params):
            return 0

        def update(self, grads, state, params=None):
            return tuple(-0.1 * g for g in grads), state + 1

    alg = bjx.meanfield_vi(recording, Descent())
    state = alg.init(torch.zeros(D, device=dev))
    key = prng.key(3)
    new, info = alg.step(key, state)
    assert recording.z.shape == (100, D) and new.opt_state == 1
    kl, g_mu, g_rho = mfvi.kl_and_grad(key, state.mu, state.rho, *recording.target(recording.z))
    assert torch.equal(new.mu, state.mu + -0.1 * g_mu) and torch.equal(new.rho, state.rho + -0.1 * g_rho)
    assert torch.equal(info.elbo, kl)
    assert alg.sample(key, new).shape == (1, D) and alg.sample(key, new, 7).shape == (7, D)
    # sgd from the package
    new, _ = mfvi.step(key, mfvi.init(torch.zeros(D, device=dev), optim.sgd(0.1)), recording, optim.sgd(0.1), 100)
    np.testing.assert_allclose(t2n(new.mu), t2n(-0.1 * g_mu), rtol=RTOL, atol=ATOL)


# ----------------------------------------------------------------------------- no host read
def test_a_step_reads_nothing_back(dev):
    """After a first step (which traces the function and compiles what it needs) two steps and a draw under
    ``torch.cuda.set_sync_debug_mode("error")`` raise nothing."""
    D = 16
    m, s = dev_t(rv.CONV_M, dev), dev_t(rv.CONV_STD, dev)

    def fn(z):
        return (-0.5 * ((z - m) / s) ** 2).sum(-1)

    algs = [bjx.meanfield_vi(fn, optim.adam(0.05), num_samples=32),
            bjx.meanfield_vi(bjx.targets.DiagGaussian(1.0 / (s * s)), optim.sgd(0.01), num_samples=32)]
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
def test_converges_on_the_diagonal_gaussian(dev):
    """The convergence case of test_meanfield_vi_api.py on the device, the target a plain PyTorch function: with STL
    the run ends inside the restatement's bounds (ten times its own worst of five keys, 2.62e-6 for ``mu`` and 9.06e-8
    for ``rho``: a floor of fp32 rounding noise), without STL it stays more than 1e-2 from the mean.  4 096 draws from the fitted approximation then have column means and standard deviations
    within 5 standard errors of the target's."""
    m, s = dev_t(rv.CONV_M, dev), dev_t(rv.CONV_STD, dev)

    def fn(z):
        return (-0.5 * ((z - m) / s) ** 2).sum(-1)

    opt = optim.adam(rv.CONV_LR)
    keys = prng.split(prng.key(rv.CONV_SEEDS[0]), rv.CONV_STEPS)
    alg = bjx.meanfield_vi(fn, opt, num_samples=rv.CONV_S)
    state = alg.init(torch.zeros(rv.CONV_D, device=dev))
    for k in keys:
        state, info = alg.step(k, state)
    err_mu, err_rho = rv.conv_errors(t2n(state.mu), t2n(state.rho))
    print("device, STL:", err_mu, err_rho, "kl", float(info.elbo))
    assert err_mu <= rv.CONV_MU_BOUND and err_rho <= rv.CONV_RHO_BOUND

    free = mfvi.init(torch.zeros(rv.CONV_D, device=dev), opt)
    for k in keys:
        free, _ = mfvi.step(k, free, fn, opt, rv.CONV_S, stl_estimator=False)
    err_free, _ = rv.conv_errors(t2n(free.mu), t2n(free.rho))
    print("device, no STL:", err_free)
    assert err_free > 1e-2

    n = 4096
    z = t2n(alg.sample(prng.key(77), state, n)).astype(f64)
    mean_err = np.abs(z.mean(0) - rv.CONV_M) / (rv.CONV_STD / np.sqrt(n))
    std_err = np.abs(z.std(0) - rv.CONV_STD) / (rv.CONV_STD / np.sqrt(2 * n))
    print("draws: worst mean and std errors in standard errors", mean_err.max(), std_err.max())
    assert mean_err.max() <= 5 and std_err.max() <= 5
