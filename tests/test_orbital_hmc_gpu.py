"""GPU parity of the periodic orbital sampler (blackjax_amd/periodic_orbital.py, csrc/bjx_orbital.hip, include/bjx_hip.h
"Periodic orbital") against the NumPy restatement of the reference's arithmetic, tests/orbital_hmc_restatement.py."""
import numpy as np
import pytest
import torch

import blackjax_amd as bjx
import orbital_hmc_restatement as ro
from blackjax_amd import integrators, periodic_orbital as po
from oracle import prng, targets as otargets
from test_mala_gpu import _gaussian_case as _mala_gaussian_case
from test_orbital_hmc_api import WEIGHT_BOUND

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


def _gaussian_case(N, P, D, per_chain, imm_per_chain=False):
    """Target, start and step size of ``test_mala_gpu._gaussian_case`` with the step divided by the period,
    0.12 D^(-1/3) / P (times uniform(0.6, 1.6) per chain), so that the far slots of the orbit keep non-negligible
    weight; the metric is a fixed diagonal, linspace(0.5, 2), times uniform(0.5, 2) per chain for the (N, D) form."""
    inv_var, q0, tau = _mala_gaussian_case(N, D, per_chain)
    eps = (tau / f32(P)).astype(f32)
    imm = np.linspace(0.5, 2.0, D).astype(f32)
    if imm_per_chain:
        imm = (imm[None, :] * np.random.default_rng(7 * N + D).uniform(0.5, 2.0, (N, 1))).astype(f32)
    return inv_var, q0, eps, imm


def _step_g(eps, per_chain, dev):
    return dev_t(eps, dev) if per_chain else float(eps)


def _assert_state(st_g, st_r):
    assert st_g.directions.dtype == torch.int32 and np.array_equal(t2n(st_g.directions), st_r.directions)
    np.testing.assert_allclose(t2n(st_g.positions), st_r.positions, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(t2n(st_g.logdensities_grad), st_r.logdensities_grad, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(t2n(st_g.logdensities), st_r.logdensities, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(t2n(st_g.weights), st_r.weights, rtol=1e-5, atol=1e-7)


def _assert_info(info_g, info_r):
    np.testing.assert_allclose(t2n(info_g.momentums), info_r.momentums, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(t2n(info_g.weights_mean), info_r.weights_mean, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(t2n(info_g.weights_variance), info_r.weights_variance, rtol=1e-5, atol=1e-7)


def _parity(dev, N, P, D, per_chain, imm_per_chain=False):
    inv_var, q0, eps, imm = _gaussian_case(N, P, D, per_chain, imm_per_chain)
    fn_r = otargets.diag_gaussian(inv_var)
    fn_g = bjx.targets.DiagGaussian(dev_t(inv_var, dev))
    eps_g, imm_g = _step_g(eps, per_chain, dev), dev_t(imm, dev)
    st_g = po.init(dev_t(q0, dev), fn_g, P)
    st_r = ro.init(q0, fn_r, P)
    _assert_state(st_g, st_r)
    chosen, heavy = [], []
    for k in prng.split(prng.key(9), 4):
        st_r, info_r, ch_r = ro.kernel(k, st_r, fn_r, eps, imm, P, chain_offset=3)
        st_g, info_g, ch_g, _ = po._transition(k, st_g, fn_g, eps_g, imm_g, P, integrators.velocity_verlet, 3)
        assert ch_g.dtype == torch.int32 and np.array_equal(t2n(ch_g), ch_r)
        _assert_state(st_g, st_r)
        _assert_info(info_g, info_r)
        assert st_g.positions.shape == (N, P, D) and st_g.weights.shape == (N, P) and info_g.weights_mean.shape == (N,)
        chosen.append(ch_r)
        heavy.append((st_r.weights > 1e-3).sum(axis=1).mean())
    chosen = np.concatenate(chosen)
    # (checked on the CPU, with the restatement) the far slots carry weight, so the select has something to choose from
    assert np.mean(heavy) >= min(2, P)
    if P > 1:  # (an orbit of one slot has nothing to choose)
        assert len(set(chosen.tolist())) >= 2 and not (chosen == 0).all()


# (N, P, D, per-chain step).  The opening kernel keeps a span of a row in registers over the P slots: 256 floats for
# the 4-byte sweep, 256 (D <= 256) or 1 024 floats for 16-byte rows; longer rows take one pass per span.  4-byte sweep
# inside one span; P = 1, D = 1; 16-byte resident in the 256-float kernel (scalar / per-chain step); 4-byte sweep beyond
# one span (whole / ragged pieces); 16-byte resident at the largest row of the 1 024-float kernel; just past it (second
# span of 8 floats); three spans with a ragged last one; prefix, select and softmax across more than one wave of slots
@pytest.mark.parametrize("N,P,D,per_chain", [(37, 5, 10, True), (5, 1, 1, False), (16, 8, 64, False), (24, 8, 64, True),
                                              (12, 3, 260, True), (7, 4, 259, True), (5, 3, 1024, True),
                                              (4, 2, 1032, False), (3, 2, 2052, True), (6, 130, 4, False)])
def test_orbital_transitions_match_restatement(dev, N, P, D, per_chain):
    """init + 4 consecutive transitions without re-sync, chain_offset = 3: chosen slots and directions exact, positions /
    gradients / log-densities / momentums within 1e-6, weights, their mean and variance within rtol 1e-5, atol 1e-7
    (the tolerances of test_mala_gpu.py)."""
    _parity(dev, N, P, D, per_chain)


def test_orbital_per_chain_inverse_mass_matrix(dev):
    """The same with one diagonal inverse mass matrix per chain, (N, D)."""
    _parity(dev, 24, 8, 64, True, imm_per_chain=True)


@pytest.mark.parametrize("eps", [0.5, 2.0])
def test_orbital_funnel_non_finite_slots(dev, eps):
    """Neal's funnel with large steps: slots whose log-weight is not finite get weight exactly 0 and no NaN reaches the
    weights (the deviation from the reference documented in the module); the selected slot stays finite."""
    N, D, P = 64, 8, 6
    q0 = (1.5 * prng.normal(prng.key(2), (N, D))).astype(f32)
    imm = np.ones(D, f32)
    fn_r = otargets.neal_funnel()
    fn_g = bjx.targets.NealFunnel()
    st_g = po.init(dev_t(q0, dev), fn_g, P)
    st_r = ro.init(q0, fn_r, P)
    rows = torch.arange(N, device=dev)
    n_zero = 0
    for k in prng.split(prng.key(4), 5):
        st_r, info_r, ch_r = ro.kernel(k, st_r, fn_r, f32(eps), imm, P)
        st_g, info_g, ch_g, _ = po._transition(k, st_g, fn_g, eps, dev_t(imm, dev), P, integrators.velocity_verlet, 0)
        assert np.array_equal(t2n(ch_g), ch_r)
        w = t2n(st_g.weights)
        assert not np.isnan(w).any()
        assert np.all(w[st_r.weights == 0] == 0)
        assert bool(torch.isfinite(st_g.weights).all()) and bool(torch.isfinite(info_g.weights_mean).all())
        assert bool(torch.isfinite(info_g.weights_variance).all())
        sel = ch_g.long()
        for x in (st_g.positions, st_g.logdensities, st_g.logdensities_grad, info_g.momentums):
            assert bool(torch.isfinite(x[rows, sel]).all())
        n_zero += int((st_r.weights == 0).sum())
    assert n_zero > 0  # the run does contain slots that were switched off


def test_orbital_is_shard_invariant(dev):
    """Chains are keyed by their GLOBAL index: chains [0, 10) and [10, 24) run with chain_offset 3 and 13 reproduce
    the unsplit run bit for bit, state and info."""
    N, P, D = 24, 8, 64
    inv_var, q0, eps, imm = _gaussian_case(N, P, D, True)
    fn = bjx.targets.DiagGaussian(dev_t(inv_var, dev))
    q0_g, eps_g, imm_g = dev_t(q0, dev), dev_t(eps, dev), dev_t(imm, dev)

    def run(lo, hi):
        alg = bjx.orbital_hmc(fn, eps_g[lo:hi].contiguous(), imm_g, P, chain_offset=3 + lo)
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


def _torch_exact_flow(imm_g, seen_steps):
    """``ro.gaussian_exact_flow`` in torch, operation for operation; records the step tensors it is handed."""

    def bijection(logdensity_fn, kinetic_energy_fn):
        def one_step(state, step_size):
            seen_steps.append(step_size)
            q, p = state.position, state.momentum
            t = step_size.double()[:, None]
            c, s = torch.cos(t).float(), torch.sin(t).float()
            q1 = q * c + (imm_g * p) * s
            p1 = p * c - (q * s) / imm_g
            logp, g = logdensity_fn.value_and_grad(q1)
            return integrators.IntegratorState(q1, p1, logp, g)

        return one_step

    return bijection


def test_orbital_callable_bijection_exact_flow(dev):
    """A bijection with the reference's signature: the exact flow of the CPU test (2 048 chains, P = 8, D = 3,
    step 2 pi / 8, 20 transitions).  Chosen slots as the restatement's, weights 1 / P within the CPU test's bound, the
    5-standard-error moment check on the device result, and the (N * P,) step tensor handed to ``one_step`` equal to
    (j - d) * step_size."""
    N, P, sigma, imm, q0, eps, keys = ro.exact_flow_case()
    inv_var = (f32(1) / imm).astype(f32)
    fn_r, fn_g = otargets.diag_gaussian(inv_var), bjx.targets.DiagGaussian(dev_t(inv_var, dev))
    imm_g = dev_t(imm, dev)
    steps = []
    kernel = po.build_kernel(_torch_exact_flow(imm_g, steps))
    flow_r = ro.gaussian_exact_flow(imm)
    st_g = po.init(dev_t(q0, dev), fn_g, P)
    st_r = ro.init(q0, fn_r, P)
    for t, k in enumerate(keys):
        st_r, info_r, ch_r = ro.kernel(k, st_r, fn_r, eps, imm, P, bijection=flow_r)
        before = st_g
        st_g, info_g = kernel(k, st_g, fn_g, float(eps), imm_g, P)
        # the chosen slot, read off the new orbit: the only slot whose signed step is 0 keeps the selected position
        step = steps[-1].view(N, P)
        ch_g = (step == 0).int().argmax(dim=1)
        assert bool(((step == 0).sum(dim=1) == 1).all()) and np.array_equal(t2n(ch_g), ch_r)
        assert same_bits(st_g.positions[torch.arange(N, device=dev), ch_g], before.positions[torch.arange(N, device=dev), ch_g])
        if t == 0:
            expect = ((np.arange(P, dtype=np.int32)[None, :] - ch_r[:, None]).astype(f32) * eps).astype(f32)
            assert steps[-1].shape == (N * P,) and np.array_equal(t2n(step), expect)
        w = t2n(st_g.weights).astype(np.float64)
        assert np.abs(w * P - 1.0).max() <= WEIGHT_BOUND
        np.testing.assert_allclose(t2n(info_g.momentums), info_r.momentums, rtol=1e-5, atol=1e-5)
    z = ro.weighted_moment_z_scores(t2n(st_g.positions), t2n(st_g.weights), sigma)
    print("z scores of the device result:", z)
    assert np.all(np.abs(z) <= 5.0), z


def test_orbital_plain_pytorch_logdensity(dev):
    """A plain PyTorch function handed to ``orbital_hmc(...)`` as is gives the chosen slots of ``targets.DiagGaussian``."""
    N, P, D = 16, 8, 64
    inv_var, q0, eps, imm = _gaussian_case(N, P, D, False)
    iv, imm_g = dev_t(inv_var, dev), dev_t(imm, dev)
    fn_p = lambda q: -0.5 * (q * q * iv).sum(-1)  # noqa: E731
    fn_t = bjx.targets.DiagGaussian(iv)
    st_p, st_t = po.init(dev_t(q0, dev), fn_p, P), po.init(dev_t(q0, dev), fn_t, P)
    chosen = []
    for k in prng.split(prng.key(9), 4):
        st_p, _, ch_p, _ = po._transition(k, st_p, fn_p, float(eps), imm_g, P, integrators.velocity_verlet, 0)
        st_t, _, ch_t, _ = po._transition(k, st_t, fn_t, float(eps), imm_g, P, integrators.velocity_verlet, 0)
        assert torch.equal(ch_p, ch_t)
        chosen.append(t2n(ch_t))
    assert len(set(np.concatenate(chosen).tolist())) >= 2
    # the traced function's gradient and fp32 row sum may round differently from the target kernel's: ulps per step
    np.testing.assert_allclose(t2n(st_p.positions), t2n(st_t.positions), rtol=1e-4, atol=1e-5)


def test_orbital_outputs_are_out_of_place_validation_and_drivers(dev):
    """``step`` leaves the tensors of the state it was given untouched; argument checks; an empty batch is a no-op;
    ``run_inference_algorithm`` stacks the orbit state and runs with chain-major keys."""
    N, P, D = 24, 8, 64
    inv_var, q0, eps, imm = _gaussian_case(N, P, D, True)
    fn = bjx.targets.DiagGaussian(dev_t(inv_var, dev))
    q0_g, eps_g, imm_g = dev_t(q0, dev), dev_t(eps, dev), dev_t(imm, dev)
    alg = bjx.orbital_hmc(fn, eps_g, imm_g, P)
    st = alg.init(q0_g)
    before = [x.clone() for x in st]
    new, info = alg.step(prng.key(9), st)
    for x, x0, y in zip(st, before, new):
        assert same_bits(x, x0) and y.data_ptr() != x.data_ptr()
    assert not same_bits(new.positions, st.positions)
    assert new.positions.shape == (N, P, D) and new.logdensities.shape == (N, P) and new.directions.shape == (N, P)
    assert new.logdensities_grad.shape == (N, P, D) and info.momentums.shape == (N, P, D)
    assert info.weights_mean.shape == (N,) and info.weights_variance.shape == (N,)

    with pytest.raises(ValueError):
        bjx.orbital_hmc(fn, torch.ones(N + 1, device=dev), imm_g, P).step(prng.key(9), st)  # wrong-length step size
    with pytest.raises(ValueError):
        bjx.orbital_hmc(fn, 0.1, imm_g, P + 1).step(prng.key(9), st)  # period does not match the state
    with pytest.raises(ValueError):
        bjx.orbital_hmc(fn, 0.1, imm_g, 0).init(q0_g)  # period < 1
    with pytest.raises(ValueError):
        bjx.orbital_hmc(fn, 0.1, imm_g, 0).step(prng.key(9), st)
    with pytest.raises(ValueError):
        alg.init(torch.zeros(D, device=dev))  # not (n_chains, dim)
    with pytest.raises(NotImplementedError):
        bjx.orbital_hmc(fn, 0.1, torch.eye(D, device=dev), P).step(prng.key(9), st)  # dense metric
    with pytest.raises(NotImplementedError):
        bjx.orbital_hmc(fn, 0.1, imm_g, P, bijection=integrators.mclachlan)  # a multi-stage Integrator
    with pytest.raises(NotImplementedError):
        po.build_kernel(integrators.yoshida)
    with pytest.raises(RuntimeError):
        alg.init(torch.zeros(3, D))  # host tensor: there is no CPU fallback
    empty_alg = bjx.orbital_hmc(fn, 0.1, imm_g, P)
    e = empty_alg.init(torch.zeros(0, D, device=dev))
    assert e.positions.shape == (0, P, D) and e.weights.shape == (0, P) and e.directions.shape == (0, P)
    e2, einfo = empty_alg.step(prng.key(1), e)
    assert e2.positions.shape == (0, P, D) and e2.weights.shape == (0, P) and e2.directions.dtype == torch.int32
    assert e2.logdensities.shape == (0, P) and e2.logdensities_grad.shape == (0, P, D)
    assert einfo.momentums.shape == (0, P, D) and einfo.weights_mean.shape == (0,) and einfo.weights_variance.shape == (0,)

    T = 3
    last, (hist_state, hist_info) = bjx.util.run_inference_algorithm(prng.key(5), alg, T, initial_position=q0_g)
    assert hist_state.positions.shape == (T, N, P, D) and hist_state.weights.shape == (T, N, P)
    assert hist_state.directions.shape == (T, N, P) and hist_info.momentums.shape == (T, N, P, D)
    assert hist_info.weights_variance.shape == (T, N) and same_bits(last.positions, hist_state.positions[-1])

    alg3 = bjx.orbital_hmc(fn, eps_g, imm_g, P, chain_offset=3)
    last, (hist_state, hist_info) = bjx.util.run_inference_algorithm(prng.key(21), alg3, T, initial_state=alg3.init(q0_g),
                                                                     key_layout="chain_major")
    fn_r = otargets.diag_gaussian(inv_var)
    st_r = ro.init(q0, fn_r, P)
    chain_keys = prng.split(prng.key(21), N, offset=3)
    for t in range(T):
        st_r, info_r, _ = ro.kernel(None, st_r, fn_r, eps, imm, P,
                                    chain_keys_override=prng.split(chain_keys, 1, offset=t)[:, 0])
        np.testing.assert_allclose(t2n(hist_state.positions[t]), st_r.positions, rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(t2n(hist_state.weights[t]), st_r.weights, rtol=1e-5, atol=1e-7)
    _assert_state(last, st_r)
    st_s, _ = alg3.step(prng.key(21), alg3.init(q0_g))  # the step-major transition of the same key differs
    assert not torch.equal(st_s.positions, hist_state.positions[0])
