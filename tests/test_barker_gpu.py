"""GPU parity of the Barker-proposal sampler (blackjax_amd/barker.py, csrc/bjx_barker.hip, include/bjx_hip.h
"Barker") and of its window adaptation against the NumPy restatement, tests/barker_restatement.py."""
import numpy as np
import pytest
import torch

import barker_restatement as rbarker
import blackjax_amd as bjx
from oracle import adaptation as oad, prng, targets as otargets

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


def _gaussian_case(N, D, per_chain, imm_kind):
    """Target, start, step size and metric of the parity cases: sigma_j = 10^(-0.5 + j / (D - 1)),
    q0 = normal(key(1)) * sigma.  ``imm_kind``: "none"; "shared" = sigma^2 (D,); "pc" = sigma^2 times
    uniform(0.5, 2) per chain and element (N, D).  tau = c D^(-1/6) -- c = 0.45 without a metric (the stiffest
    sigma is 0.32), 1.4 with one -- times uniform(0.6, 1.6) per chain."""
    sig = (10.0 ** (-0.5 + 1.0 * np.arange(D) / max(D - 1, 1))).astype(f32)
    inv_var = (f32(1) / (sig * sig)).astype(f32)
    q0 = (prng.normal(prng.key(1), (N, D)) * sig).astype(f32)
    rng = np.random.default_rng(100 * N + D)
    tau = f32((0.45 if imm_kind == "none" else 1.4) * D ** (-1.0 / 6.0))
    if per_chain:
        tau = (tau * rng.uniform(0.6, 1.6, N)).astype(f32)
    imm = None
    if imm_kind == "shared":
        imm = (sig * sig).astype(f32)
    elif imm_kind == "pc":
        imm = ((sig * sig) * rng.uniform(0.5, 2.0, (N, D))).astype(f32)
    return inv_var, q0, tau, imm


def _imm_arg(imm, dev):
    if imm is None:
        return None
    return bjx.metrics.PerChainDiag(dev_t(imm, dev)) if imm.ndim == 2 else dev_t(imm, dev)


def _assert_state(st_g, st_r):
    np.testing.assert_allclose(t2n(st_g.position), st_r.position, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(t2n(st_g.logdensity_grad), st_r.logdensity_grad, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(t2n(st_g.logdensity), st_r.logdensity, rtol=1e-6, atol=1e-6)


PARITY_CASES = [(37, 10, True, "pc"), (5, 1, False, "none"), (16, 64, False, "shared"), (24, 64, True, "pc"),
                (33, 260, True, "none"), (7, 259, True, "shared"), (9, 1024, True, "pc"), (6, 1032, False, "shared"),
                (3, 2052, True, "none")]


# (N, D, per-chain tau, metric): 4-byte sweep; 4-byte sweep, one element; 16-byte resident NI = 1 (scalar / per-chain
# tau); resident NI = 2; 4-byte sweep beyond one 256-float span; resident NI = 4 at its largest row; 16-byte two-pass
# just past the resident limit; 16-byte two-pass with a ragged last span.  Each metric form on three shapes, a scalar
# step size on three, a per-chain one on six.
@pytest.mark.parametrize("N,D,per_chain,imm_kind", PARITY_CASES)
def test_barker_transitions_match_restatement(dev, N, D, per_chain, imm_kind):
    """init + 6 consecutive transitions without re-sync, chain_offset = 3: accept bits exact, positions / gradients /
    log-densities of the state and of the proposal within 1e-6, acceptance rates within rtol 1e-5 (the tolerances of
    test_mala_gpu.py and test_ghmc_gpu.py); the per-element signs of the first transition, taken from identical
    inputs, are those of the restatement wherever the increment is not zero."""
    inv_var, q0, tau, imm = _gaussian_case(N, D, per_chain, imm_kind)
    fn_r = otargets.diag_gaussian(inv_var)
    alg = bjx.barker(bjx.targets.DiagGaussian(dev_t(inv_var, dev)), dev_t(tau, dev) if per_chain else float(tau),
                     _imm_arg(imm, dev), chain_offset=3)
    st_g = alg.init(dev_t(q0, dev))
    st_r = rbarker.init(q0, fn_r)
    _assert_state(st_g, st_r)
    st_g = type(st_g)(*[dev_t(x, dev) for x in st_r])  # identical inputs for the first transition
    keys = prng.split(prng.key(9), 6)
    q1_r, b_r, z_r = rbarker.propose(prng.split(keys[0], N, offset=3), st_r.position, st_r.logdensity_grad, tau, imm)
    n_acc = 0
    for t, k in enumerate(keys):
        q_before = st_r.position
        st_r, info_r = rbarker.kernel(k, st_r, fn_r, tau, imm, chain_offset=3)
        st_g, info_g = alg.step(k, st_g)
        assert info_g.is_accepted.dtype == torch.bool and info_g.acceptance_rate.dtype == torch.float32
        if t == 0:
            moved = z_r != 0
            assert moved.any() and 0 < int(b_r.sum()) < b_r.size
            sign_g = np.sign(t2n(info_g.proposal.position) - q_before)
            assert np.array_equal(sign_g[moved], np.sign(q1_r - q_before)[moved])
        assert np.array_equal(t2n(info_g.is_accepted), info_r.is_accepted)
        np.testing.assert_allclose(t2n(info_g.acceptance_rate), info_r.acceptance_rate, rtol=1e-5, atol=1e-7)
        _assert_state(st_g, st_r)
        _assert_state(info_g.proposal, info_r.proposal)
        n_acc += int(info_r.is_accepted.sum())
    assert 0 < n_acc < 6 * N  # both branches of the select were exercised at this shape


@pytest.mark.parametrize("tau_even,tau_odd", [(1.0, 60.0), (2.0, 100.0)])
def test_barker_funnel_non_finite_proposals(dev, tau_even, tau_odd):
    """Neal's funnel with large steps (the odd chains take steps of 60 or 100, far enough down the neck that
    exp(-y) overflows; the even ones moderate steps, so that accepts occur too): proposals whose log-density or ratio
    is not finite are rejected with an acceptance rate of exactly 0 (never NaN), as safe_energy_diff prescribes; the
    state stays finite."""
    N, D = 64, 8
    q0 = (1.5 * prng.normal(prng.key(2), (N, D))).astype(f32)
    tau_np = np.where(np.arange(N) % 2 == 0, tau_even, tau_odd).astype(f32)
    fn_r = otargets.neal_funnel()
    alg = bjx.barker(bjx.targets.NealFunnel(), dev_t(tau_np, dev))
    st_g = alg.init(dev_t(q0, dev))
    st_r = rbarker.init(q0, fn_r)
    n_acc = n_bad = 0
    for k in prng.split(prng.key(4), 5):
        st_r, info_r = rbarker.kernel(k, st_r, fn_r, tau_np)
        st_g, info_g = alg.step(k, st_g)
        rate = t2n(info_g.acceptance_rate)
        assert np.array_equal(t2n(info_g.is_accepted), info_r.is_accepted)
        assert not np.isnan(rate).any()
        assert np.all(rate[info_r.acceptance_rate == 0] == 0)
        bad = ~np.isfinite(info_r.proposal.logdensity) | ~np.isfinite(info_r.proposal.logdensity_grad).all(-1)
        assert np.all(rate[bad] == 0) and not t2n(info_g.is_accepted)[bad].any()
        for x in st_g:
            assert bool(torch.isfinite(x).all())
        n_acc += int(info_r.is_accepted.sum())
        n_bad += int(bad.sum())
    assert 0 < n_acc < 5 * N and n_bad > 0  # the case does contain accepted, rejected and non-finite proposals


def test_barker_is_shard_invariant_and_chain_major(dev):
    """Chains are keyed by their GLOBAL index: chains [0, 10) and [10, 24) run with chain_offset 3 and 13 reproduce
    the unsplit run bit for bit.  A chain-major key through run_inference_algorithm equals the restatement driven
    with chain i's keys split(split(key, .)[3 + i], .)[t]."""
    N, D = 24, 64
    inv_var, q0, tau, imm = _gaussian_case(N, D, True, "pc")
    fn = bjx.targets.DiagGaussian(dev_t(inv_var, dev))
    q0_g, tau_g, imm_g = dev_t(q0, dev), dev_t(tau, dev), dev_t(imm, dev)

    def run(lo, hi):
        alg = bjx.barker(fn, tau_g[lo:hi].contiguous(), bjx.metrics.PerChainDiag(imm_g[lo:hi].contiguous()),
                         chain_offset=3 + lo)
        st = alg.init(q0_g[lo:hi].contiguous())
        for k in prng.split(prng.key(9), 6):
            st, info = alg.step(k, st)
        return st, info

    full, info_full = run(0, N)
    a, info_a = run(0, 10)
    b, info_b = run(10, N)
    for f, x, y in zip(full, a, b):
        assert same_bits(f, torch.cat([x, y]))
    for f, x, y in zip(info_full[:2] + tuple(info_full.proposal), info_a[:2] + tuple(info_a.proposal),
                       info_b[:2] + tuple(info_b.proposal)):
        assert same_bits(f, torch.cat([x, y]))

    T = 4
    alg = bjx.barker(fn, tau_g, bjx.metrics.PerChainDiag(imm_g), chain_offset=3)
    st_g, (hist_state, hist_info) = bjx.util.run_inference_algorithm(prng.key(21), alg, T, initial_state=alg.init(q0_g),
                                                                     key_layout="chain_major")
    fn_r = otargets.diag_gaussian(inv_var)
    st_r = rbarker.init(q0, fn_r)
    chain_keys = prng.split(prng.key(21), N, offset=3)
    for t in range(T):
        st_r, info_r = rbarker.kernel(None, st_r, fn_r, tau, imm,
                                      chain_keys_override=prng.split(chain_keys, 1, offset=t)[:, 0])
        assert np.array_equal(t2n(hist_info.is_accepted[t]), info_r.is_accepted)
        np.testing.assert_allclose(t2n(hist_state.position[t]), st_r.position, rtol=1e-6, atol=1e-6)
    _assert_state(st_g, st_r)
    # and the chain-major transitions differ from the step-major ones of the same key
    st_s, _ = alg.step(prng.key(21), alg.init(q0_g))
    assert not torch.equal(st_s.position, hist_state.position[0])


def test_barker_plain_pytorch_logdensity(dev):
    """A plain PyTorch function handed to ``barker(...)`` as is gives the accept bits of ``targets.DiagGaussian``."""
    N, D = 16, 64
    inv_var, q0, tau, imm = _gaussian_case(N, D, False, "shared")
    iv = dev_t(inv_var, dev)
    alg_p = bjx.barker(lambda q: -0.5 * (q * q * iv).sum(-1), float(tau), dev_t(imm, dev))
    alg_t = bjx.barker(bjx.targets.DiagGaussian(iv), float(tau), dev_t(imm, dev))
    st_p, st_t = alg_p.init(dev_t(q0, dev)), alg_t.init(dev_t(q0, dev))
    n_acc = 0
    for k in prng.split(prng.key(9), 6):
        st_p, info_p = alg_p.step(k, st_p)
        st_t, info_t = alg_t.step(k, st_t)
        assert torch.equal(info_p.is_accepted, info_t.is_accepted)
        n_acc += int(info_t.is_accepted.sum())
    assert 0 < n_acc < 6 * N
    # the traced function's gradient and fp32 row sum may round differently from the target kernel's: ulps per step
    np.testing.assert_allclose(t2n(st_p.position), t2n(st_t.position), rtol=1e-4, atol=1e-5)


def test_barker_outputs_are_out_of_place_and_validation(dev):
    """``step`` leaves the tensors of the state it was given untouched; argument checks; an empty batch is a no-op;
    a dense metric is refused by name, a metric of the wrong length is a ValueError."""
    N, D = 24, 64
    inv_var, q0, tau, imm = _gaussian_case(N, D, True, "pc")
    fn = bjx.targets.DiagGaussian(dev_t(inv_var, dev))
    alg = bjx.barker(fn, dev_t(tau, dev), bjx.metrics.PerChainDiag(dev_t(imm, dev)))
    st = alg.init(dev_t(q0, dev))
    before = [x.clone() for x in st]
    new, info = alg.step(prng.key(9), st)
    for x, x0, y in zip(st, before, new):
        assert same_bits(x, x0) and y.data_ptr() != x.data_ptr()
    for x, y in zip(st, info.proposal):
        assert y.data_ptr() != x.data_ptr()
    assert bool(info.is_accepted.any()) and not same_bits(new.position, st.position)
    assert new.position.shape == (N, D) and new.logdensity.shape == (N,) and info.acceptance_rate.shape == (N,)
    assert info.proposal.position.shape == (N, D) and info.proposal.logdensity.shape == (N,)

    key = prng.key(9)
    for dense in (torch.eye(D, device=dev), torch.eye(D, device=dev).expand(N, D, D).contiguous(),
                  bjx.metrics.Metric("dense", torch.eye(D, device=dev), 0, torch.eye(D, device=dev))):
        with pytest.raises(NotImplementedError, match="diagonal"):
            bjx.barker(fn, 0.1, dense).step(key, st)
    with pytest.raises(ValueError):
        bjx.barker(fn, 0.1, torch.ones(D + 1, device=dev)).step(key, st)  # shared diagonal of the wrong length
    with pytest.raises(ValueError):
        bjx.barker(fn, 0.1, bjx.metrics.PerChainDiag(torch.ones(N, D + 4, device=dev))).step(key, st)
    with pytest.raises(ValueError):
        bjx.barker(fn, torch.ones(N + 1, device=dev)).step(key, st)  # per-chain step size of the wrong length
    with pytest.raises(ValueError):
        alg.init(torch.zeros(D, device=dev))  # not (n_chains, dim)
    with pytest.raises(RuntimeError):
        alg.init(torch.zeros(3, D))  # host tensor: there is no CPU fallback
    # a diagonal metrics.Metric is taken as it is
    m = bjx.metrics.default_metric(dev_t(imm, dev), N, D, dev)
    new_m, info_m = bjx.barker(fn, dev_t(tau, dev), m).step(key, st)
    assert same_bits(new_m.position, new.position) and same_bits(info_m.acceptance_rate, info.acceptance_rate)
    e = bjx.barker(fn, 0.1).init(torch.zeros(0, D, device=dev))
    e2, einfo = bjx.barker(fn, 0.1, torch.ones(D, device=dev)).step(prng.key(1), e)
    assert e2.position.shape == (0, D) and einfo.is_accepted.shape == (0,)
    assert einfo.proposal.position.shape == (0, D)

    last, (hist_state, hist_info) = bjx.util.run_inference_algorithm(prng.key(5), bjx.barker(fn, 0.01), 3,
                                                                     initial_position=dev_t(q0, dev))
    assert hist_state.position.shape == (3, N, D) and hist_info.is_accepted.shape == (3, N)
    assert same_bits(last.position, hist_state.position[-1])


@pytest.mark.parametrize("N,D", [(12, 16), (5, 259)])
def test_barker_window_adaptation_matches_restatement(dev, N, D):
    """window_adaptation(barker, ...).run over 120 steps (the Stan schedule then holds one window end, at step 107)
    against oracle.adaptation.window_adaptation_run driving the restated kernel: every step's accept bits exact, the
    final step sizes and inverse mass matrices within rtol 1e-6 (the tolerances test_adaptation_gpu.py states for
    HMC); the returned parameters then construct a sampler that steps from the returned state."""
    num_steps = 120
    assert any(end for _, end in oad.build_schedule(num_steps))
    inv_var, q0, _, _ = _gaussian_case(N, D, False, "none")
    fn_r = otargets.diag_gaussian(inv_var)
    accepts = []

    def kernel_fn(keys_t, state, step_size, imm):
        st, info = rbarker.kernel(None, rbarker.BarkerState(*state), fn_r, step_size, imm, chain_keys_override=keys_t)
        accepts.append(info.is_accepted)
        return st, info

    run_key = prng.key(19)
    eps0 = 0.3
    st_o, par_o, hist_o = oad.window_adaptation_run(run_key, q0, fn_r, num_steps, None, initial_step_size=eps0,
                                                    target_acceptance_rate=0.4, kernel_fn=kernel_fn)
    fn = bjx.targets.DiagGaussian(dev_t(inv_var, dev))
    warm = bjx.window_adaptation(bjx.barker, fn, target_acceptance_rate=0.4, initial_step_size=eps0)
    (st_g, par_g), info = warm.run(run_key, dev_t(q0, dev), num_steps)
    isacc_g = t2n(info.info.is_accepted)
    acc_g = t2n(info.info.acceptance_rate)
    assert isacc_g.shape == (num_steps, N)
    for t in range(num_steps):
        assert np.array_equal(isacc_g[t], accepts[t]), t
        np.testing.assert_allclose(acc_g[t], hist_o[t][0], rtol=1e-5, atol=1e-7)
    assert 0 < int(isacc_g.sum()) < isacc_g.size
    np.testing.assert_allclose(t2n(par_g["step_size"]), par_o["step_size"], rtol=1e-6)
    assert isinstance(par_g["inverse_mass_matrix"], bjx.metrics.PerChainDiagTensor)
    assert par_g["inverse_mass_matrix"].shape == (N, D)
    np.testing.assert_allclose(t2n(par_g["inverse_mass_matrix"]),
                               np.broadcast_to(par_o["inverse_mass_matrix"], (N, D)), rtol=1e-6)
    _assert_state(st_g, st_o)
    assert set(par_g) == {"step_size", "inverse_mass_matrix"}
    new, info1 = bjx.barker(fn, **par_g).step(prng.key(3), st_g)
    st_r, info_r = rbarker.kernel(prng.key(3), rbarker.BarkerState(*st_o), fn_r, par_o["step_size"],
                                  par_o["inverse_mass_matrix"])
    assert np.array_equal(t2n(info1.is_accepted), info_r.is_accepted)
    _assert_state(new, st_r)


def test_barker_window_adaptation_argument_errors(dev):
    fn = bjx.targets.DiagGaussian(torch.ones(8, device=dev))
    with pytest.raises(ValueError, match="integrator"):
        bjx.window_adaptation(bjx.barker, fn, integrator=bjx.integrators.mclachlan)
    with pytest.raises(NotImplementedError):
        bjx.window_adaptation(bjx.barker, fn, is_mass_matrix_diagonal=False)
    with pytest.raises(NotImplementedError):
        bjx.window_adaptation(bjx.barker, fn, fuse_target=True)
    warm = bjx.window_adaptation(bjx.barker_proposal, fn)
    with pytest.raises(NotImplementedError):
        warm.run(prng.key(1), torch.zeros(4, 8, device=dev), 30, free_running=True)
