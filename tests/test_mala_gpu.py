"""GPU parity of the Metropolis-adjusted Langevin sampler (blackjax_amd/mala.py, csrc/bjx_mala.hip,
include/bjx_hip.h "MALA") against the NumPy restatement of the reference's arithmetic, tests/mala_restatement.py."""
import numpy as np
import pytest
import torch

import blackjax_amd as bjx
import mala_restatement as rmala
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


def _gaussian_case(N, D, per_chain):
    """Target, start and step size of the parity cases: sigma_j = 10^(-0.5 + j / (D - 1)), q0 = normal(key(1)) * sigma,
    tau = 0.12 D^(-1/3), times uniform(0.6, 1.6) per chain."""
    sig = (10.0 ** (-0.5 + 1.0 * np.arange(D) / max(D - 1, 1))).astype(f32)
    inv_var = (f32(1) / (sig * sig)).astype(f32)
    q0 = (prng.normal(prng.key(1), (N, D)) * sig).astype(f32)
    tau = f32(0.12 * D ** (-1.0 / 3.0))
    if per_chain:
        tau = (tau * np.random.default_rng(100 * N + D).uniform(0.6, 1.6, N)).astype(f32)
    return inv_var, q0, tau


def _assert_state(st_g, st_r):
    np.testing.assert_allclose(t2n(st_g.position), st_r.position, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(t2n(st_g.logdensity_grad), st_r.logdensity_grad, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(t2n(st_g.logdensity), st_r.logdensity, rtol=1e-6, atol=1e-6)


# (N, D, per-chain tau): 4-byte sweep; 4-byte sweep, one element; 16-byte resident NI = 1 (scalar / per-chain tau);
# resident NI = 2; 4-byte sweep beyond one 256-float span; resident NI = 4 at its largest row; 16-byte two-pass just
# past the resident limit; 16-byte two-pass with a ragged last span
@pytest.mark.parametrize("N,D,per_chain", [(37, 10, True), (5, 1, False), (16, 64, False), (24, 64, True),
                                            (33, 260, True), (7, 259, True), (9, 1024, True), (6, 1032, False),
                                            (3, 2052, True)])
def test_mala_transitions_match_restatement(dev, N, D, per_chain):
    """init + 6 consecutive transitions without re-sync, chain_offset = 3: accept bits exact, positions / gradients /
    log-densities within 1e-6, acceptance rates within rtol 1e-5 (the tolerances of test_ghmc_gpu.py)."""
    inv_var, q0, tau = _gaussian_case(N, D, per_chain)
    fn_r = otargets.diag_gaussian(inv_var)
    alg = bjx.mala(bjx.targets.DiagGaussian(dev_t(inv_var, dev)), dev_t(tau, dev) if per_chain else float(tau),
                   chain_offset=3)
    st_g = alg.init(dev_t(q0, dev))
    st_r = rmala.init(q0, fn_r)
    _assert_state(st_g, st_r)
    n_acc = 0
    for k in prng.split(prng.key(9), 6):
        st_r, info_r = rmala.kernel(k, st_r, fn_r, tau, chain_offset=3)
        st_g, info_g = alg.step(k, st_g)
        assert info_g.is_accepted.dtype == torch.bool and info_g.acceptance_rate.dtype == torch.float32
        assert np.array_equal(t2n(info_g.is_accepted), info_r.is_accepted)
        np.testing.assert_allclose(t2n(info_g.acceptance_rate), info_r.acceptance_rate, rtol=1e-5, atol=1e-7)
        _assert_state(st_g, st_r)
        n_acc += int(info_r.is_accepted.sum())
    assert 0 < n_acc < 6 * N  # both branches of the select were exercised at this shape


@pytest.mark.parametrize("tau", [0.5, 2.0])
def test_mala_funnel_non_finite_proposals(dev, tau):
    """Neal's funnel with large steps: proposals whose log-density or transition energy is not finite are rejected
    with an acceptance rate of exactly 0 (never NaN), as safe_energy_diff prescribes; the state stays finite."""
    N, D = 64, 8
    q0 = (1.5 * prng.normal(prng.key(2), (N, D))).astype(f32)
    fn_r = otargets.neal_funnel()
    alg = bjx.mala(bjx.targets.NealFunnel(), tau)
    st_g = alg.init(dev_t(q0, dev))
    st_r = rmala.init(q0, fn_r)
    n_acc = n_zero = 0
    for k in prng.split(prng.key(4), 5):
        st_r, info_r = rmala.kernel(k, st_r, fn_r, tau)
        st_g, info_g = alg.step(k, st_g)
        rate = t2n(info_g.acceptance_rate)
        assert np.array_equal(t2n(info_g.is_accepted), info_r.is_accepted)
        assert not np.isnan(rate).any()
        assert np.all(rate[info_r.acceptance_rate == 0] == 0)
        for x in st_g:
            assert bool(torch.isfinite(x).all())
        n_acc += int(info_r.is_accepted.sum())
        n_zero += int((info_r.acceptance_rate == 0).sum())
    assert 0 < n_acc < 5 * N and n_zero > 0  # the case does contain accepted, rejected and non-finite proposals


def test_mala_is_shard_invariant_and_chain_major(dev):
    """Chains are keyed by their GLOBAL index: chains [0, 10) and [10, 24) run with chain_offset 3 and 13 reproduce
    the unsplit run bit for bit.  A chain-major key through run_inference_algorithm equals the restatement driven
    with chain i's keys split(split(key, .)[3 + i], .)[t]."""
    N, D = 24, 64
    inv_var, q0, tau = _gaussian_case(N, D, True)
    fn = bjx.targets.DiagGaussian(dev_t(inv_var, dev))
    q0_g, tau_g = dev_t(q0, dev), dev_t(tau, dev)

    def run(lo, hi):
        alg = bjx.mala(fn, tau_g[lo:hi].contiguous(), chain_offset=3 + lo)
        st = alg.init(q0_g[lo:hi].contiguous())
        for k in prng.split(prng.key(9), 6):
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
    alg = bjx.mala(fn, tau_g, chain_offset=3)
    st_g, (hist_state, hist_info) = bjx.util.run_inference_algorithm(prng.key(21), alg, T, initial_state=alg.init(q0_g),
                                                                     key_layout="chain_major")
    fn_r = otargets.diag_gaussian(inv_var)
    st_r = rmala.init(q0, fn_r)
    chain_keys = prng.split(prng.key(21), N, offset=3)
    for t in range(T):
        st_r, info_r = rmala.kernel(None, st_r, fn_r, tau, chain_keys_override=prng.split(chain_keys, 1, offset=t)[:, 0])
        assert np.array_equal(t2n(hist_info.is_accepted[t]), info_r.is_accepted)
        np.testing.assert_allclose(t2n(hist_state.position[t]), st_r.position, rtol=1e-6, atol=1e-6)
    _assert_state(st_g, st_r)
    # and the chain-major transitions differ from the step-major ones of the same key
    st_s, _ = alg.step(prng.key(21), alg.init(q0_g))
    assert not torch.equal(st_s.position, hist_state.position[0])


def test_mala_plain_pytorch_logdensity(dev):
    """A plain PyTorch function handed to ``mala(...)`` as is gives the accept bits of ``targets.DiagGaussian``."""
    N, D = 16, 64
    inv_var, q0, tau = _gaussian_case(N, D, False)
    iv = dev_t(inv_var, dev)
    alg_p = bjx.mala(lambda q: -0.5 * (q * q * iv).sum(-1), float(tau))
    alg_t = bjx.mala(bjx.targets.DiagGaussian(iv), float(tau))
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


def test_mala_outputs_are_out_of_place_and_validation(dev):
    """``step`` leaves the tensors of the state it was given untouched; argument checks; an empty batch is a no-op;
    ``run_inference_algorithm(initial_position=...)`` works (``init`` takes and ignores an rng_key)."""
    N, D = 24, 64
    inv_var, q0, tau = _gaussian_case(N, D, True)
    fn = bjx.targets.DiagGaussian(dev_t(inv_var, dev))
    alg = bjx.mala(fn, dev_t(tau, dev))
    st = alg.init(dev_t(q0, dev))
    before = [x.clone() for x in st]
    new, info = alg.step(prng.key(9), st)
    for x, x0, y in zip(st, before, new):
        assert same_bits(x, x0) and y.data_ptr() != x.data_ptr()
    assert bool(info.is_accepted.any()) and not same_bits(new.position, st.position)
    assert new.position.shape == (N, D) and new.logdensity.shape == (N,) and info.acceptance_rate.shape == (N,)

    with pytest.raises(ValueError):
        bjx.mala(fn, torch.ones(N + 1, device=dev)).step(prng.key(9), st)  # per-chain step size of the wrong length
    with pytest.raises(ValueError):
        alg.init(torch.zeros(D, device=dev))  # not (n_chains, dim)
    with pytest.raises(RuntimeError):
        alg.init(torch.zeros(3, D))  # host tensor: there is no CPU fallback
    e = bjx.mala(fn, 0.1).init(torch.zeros(0, D, device=dev))
    e2, einfo = bjx.mala(fn, 0.1).step(prng.key(1), e)
    assert e2.position.shape == (0, D) and einfo.is_accepted.shape == (0,)

    last, (hist_state, hist_info) = bjx.util.run_inference_algorithm(prng.key(5), bjx.mala(fn, 0.01), 3,
                                                                     initial_position=dev_t(q0, dev))
    assert hist_state.position.shape == (3, N, D) and hist_info.is_accepted.shape == (3, N)
    assert same_bits(last.position, hist_state.position[-1])
