"""GPU parity of the random-walk Metropolis family (blackjax_amd/random_walk.py, irmh.py, csrc/bjx_rw.hip,
include/bjx_hip.h "random walk") against the NumPy restatement of the reference's arithmetic,
tests/random_walk_restatement.py."""
import numpy as np
import pytest
import torch

import blackjax_amd as bjx
import random_walk_restatement as rrw
import smc_restatement as rsmc
from blackjax_amd import random_walk as prw
from blackjax_amd import smc
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


def _gaussian_case(N, D):
    """Target and start of the parity cases, those of test_mala_gpu._gaussian_case: sigma_j = 10^(-0.5 + j / (D - 1)),
    q0 = normal(key(1)) * sigma."""
    sig = (10.0 ** (-0.5 + 1.0 * np.arange(D) / max(D - 1, 1))).astype(f32)
    inv_var = (f32(1) / (sig * sig)).astype(f32)
    q0 = (prng.normal(prng.key(1), (N, D)) * sig).astype(f32)
    return sig, inv_var, q0


def _sigma(kind, D, sig):
    """The step of a parity case: 2.4 / sqrt(D) times the target scale (diag), its mean (scalar), or a lower-triangular
    matrix of that size (dense: not symmetric, so ``sigma @ z`` and ``z @ sigma`` differ)."""
    c = 2.4 / np.sqrt(D)
    if kind == "scalar":
        return f32(c * sig.mean())
    if kind == "diag":
        return (f32(c) * sig).astype(f32)
    chol = np.linalg.cholesky(otargets.ar1_covariance(0.7, D).astype(np.float64))
    return (c * sig.astype(np.float64)[:, None] * chol).astype(f32)


def _sigma_arg(sigma, dev):
    return float(sigma) if np.ndim(sigma) == 0 else dev_t(sigma, dev)


def _assert_state(st_g, st_r):
    np.testing.assert_allclose(t2n(st_g.position), st_r.position, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(t2n(st_g.logdensity), st_r.logdensity, rtol=1e-6, atol=1e-6)


def _assert_transition(st_g, info_g, st_r, info_r):
    assert info_g.is_accepted.dtype == torch.bool and info_g.acceptance_rate.dtype == torch.float32
    assert np.array_equal(t2n(info_g.is_accepted), info_r.is_accepted)
    np.testing.assert_allclose(t2n(info_g.acceptance_rate), info_r.acceptance_rate, rtol=1e-5, atol=1e-7)
    _assert_state(st_g, st_r)
    _assert_state(info_g.proposal, info_r.proposal)


def _restatement_run(N, D, kind, run_key, n_steps=6, chain_offset=3):
    """init + ``n_steps`` transitions of the restatement: [(state, info)], the first entry (state, None)."""
    sig, inv_var, q0 = _gaussian_case(N, D)
    fn_r = otargets.diag_gaussian(inv_var)
    step = rrw.normal(_sigma(kind, D, sig))
    st = rrw.init(q0, fn_r)
    out = [(st, None)]
    for k in prng.split(prng.key(run_key), n_steps):
        st, info = rrw.additive_step_kernel(k, st, fn_r, step, chain_offset=chain_offset)
        out.append((st, info))
    return out


# (N, D, sigma kind, run key): 4-byte sweep, one element; 4-byte sweep; 16-byte sweep (scalar / diag); 4-byte sweep
# past one 256-float span; 16-byte sweep with a ragged last span (diag / scalar); dense: 4-byte, 16-byte, and the
# ragged shape of test_elliptical_slice_gpu's dense cases (D no multiple of the GEMM's 16-wide k tile).  With the run
# key given, the restatement alone accepts some and rejects some of each case's 6 N proposals (checked on the CPU).
PARITY_CASES = [(5, 1, "scalar", 9), (37, 10, "diag", 9), (16, 64, "scalar", 9), (24, 64, "diag", 9),
                (7, 259, "diag", 9), (6, 1032, "diag", 9), (3, 2052, "scalar", 2),
                (9, 8, "dense", 9), (24, 64, "dense", 9), (24, 20, "dense", 9)]


@pytest.mark.parametrize("N,D,kind,run_key", PARITY_CASES)
def test_random_walk_transitions_match_restatement(dev, N, D, kind, run_key):
    """init + 6 consecutive transitions of normal_random_walk without re-sync, chain_offset = 3: accept bits exact,
    positions / log-densities / the proposal of ``info`` within 1e-6, acceptance rates within rtol 1e-5 (the tolerances
    of test_mala_gpu.py; the dense cases restate the MFMA GEMM as the fp32 fma chain in the engine's k order and keep
    the 1e-6 of the dense elliptical-slice cases)."""
    sig, inv_var, q0 = _gaussian_case(N, D)
    ref = _restatement_run(N, D, kind, run_key)
    alg = bjx.normal_random_walk(bjx.targets.DiagGaussian(dev_t(inv_var, dev)), _sigma_arg(_sigma(kind, D, sig), dev),
                                 chain_offset=3)
    st_g = alg.init(dev_t(q0, dev))
    _assert_state(st_g, ref[0][0])
    n_acc = 0
    for k, (st_r, info_r) in zip(prng.split(prng.key(run_key), 6), ref[1:]):
        st_g, info_g = alg.step(k, st_g)
        _assert_transition(st_g, info_g, st_r, info_r)
        n_acc += int(info_r.is_accepted.sum())
    assert 0 < n_acc < 6 * N  # both branches of the select were exercised at this shape


@pytest.mark.parametrize("N,D", [(24, 64), (7, 259)])
def test_chain_normal_is_bit_equal_to_the_oracle(dev, N, D):
    """Row i of ``random.chain_normal`` is ``normal(k, (D,))`` of chain i's key, or of a child of its 2-way split, bit
    for bit; step-major and chain-major keys, 16-byte and 4-byte sweeps."""
    run = prng.key(17)
    for rng_key, keys in ((run, prng.split(run, N, offset=3)),
                          (bjx.random.ChainMajorKey(run, 5), prng.split(prng.split(run, N, offset=3), 1, offset=5)[:, 0])):
        for child in (None, 0, 1):
            z = bjx.random.chain_normal(rng_key, N, D, device=dev, chain_offset=3, child=child)
            assert z.shape == (N, D) and z.dtype == torch.float32 and z.is_cuda
            assert np.array_equal(t2n(z).view(np.int32), rrw.chain_normal(keys, D, child).view(np.int32)), child
    assert bjx.random.chain_normal(run, 0, D, device=dev).shape == (0, D)
    with pytest.raises(ValueError):
        bjx.random.chain_normal(run, N, D, device=dev, child=2)
    with pytest.raises(RuntimeError):
        bjx.random.chain_normal(run, N, D, device="cpu")


def _asymmetric_case(dev):
    """N, D = 24, 64: a drifting rmh proposal q1 = q0 + drift + s z and an independent irmh proposal 1.1 sigma z, both
    drawing z from ``key_proposal`` through chain_normal(child=0); the proposal log-densities are summed in fp64 and
    rounded once on both sides."""
    N, D = 24, 64
    sig, inv_var, q0 = _gaussian_case(N, D)
    s = (f32(2.4 / np.sqrt(D)) * sig).astype(f32)
    drift = (f32(0.05) * sig).astype(f32)
    wide = (f32(1.1) * sig).astype(f32)
    s_g, drift_g, wide_g = dev_t(s, dev), dev_t(drift, dev), dev_t(wide, dev)

    def gen_g(rng_key, position):
        z = bjx.random.chain_normal(rng_key, N, D, device=dev, chain_offset=3, child=0)
        return (position + drift_g) + s_g * z

    def gen_r(rng_key, keys, position):
        return ((position + drift).astype(f32) + (s * rrw.chain_normal(keys, D, 0)).astype(f32)).astype(f32)

    def f_rmh_g(a, b):
        r = (b.position.double() - a.position.double() - drift_g.double()) / s_g.double()
        return (-0.5 * (r * r).sum(-1)).float()

    def f_rmh_r(a, b):
        r = (b.position.astype(np.float64) - a.position.astype(np.float64) - drift.astype(np.float64)) / s.astype(np.float64)
        return (-0.5 * np.sum(r * r, axis=-1)).astype(f32)

    def draw_g(rng_key):
        return wide_g * bjx.random.chain_normal(rng_key, N, D, device=dev, chain_offset=3, child=0)

    def draw_r(rng_key, keys):
        return (wide * rrw.chain_normal(keys, D, 0)).astype(f32)

    def f_irmh_g(a, b):
        r = b.position.double() / wide_g.double()
        return (-0.5 * (r * r).sum(-1)).float()

    def f_irmh_r(a, b):
        r = b.position.astype(np.float64) / wide.astype(np.float64)
        return (-0.5 * np.sum(r * r, axis=-1)).astype(f32)

    return inv_var, q0, (gen_g, f_rmh_g, gen_r, f_rmh_r), (draw_g, f_irmh_g, draw_r, f_irmh_r)


@pytest.mark.parametrize("which", ["rmh", "irmh"])
def test_asymmetric_proposals_match_restatement(dev, which):
    """rmh with a drifting proposal and irmh with an over-dispersed independent one, each with its matching
    ``proposal_logdensity_fn``: 6 transitions against the restatement to the tolerances of the parity cases."""
    inv_var, q0, rmh_case, irmh_case = _asymmetric_case(dev)
    fn_r = otargets.diag_gaussian(inv_var)
    fn_g = bjx.targets.DiagGaussian(dev_t(inv_var, dev))
    if which == "rmh":
        gen_g, f_g, gen_r, f_r = rmh_case
        alg, kernel_r = bjx.rmh(fn_g, gen_g, f_g, chain_offset=3), rrw.rmh_kernel
    else:
        gen_g, f_g, gen_r, f_r = irmh_case
        alg, kernel_r = bjx.irmh(fn_g, gen_g, f_g, chain_offset=3), rrw.irmh_kernel
    st_g, st_r = alg.init(dev_t(q0, dev)), rrw.init(q0, fn_r)
    n_acc = 0
    for k in prng.split(prng.key(9), 6):
        st_r, info_r = kernel_r(k, st_r, fn_r, gen_r, f_r, chain_offset=3)
        st_g, info_g = alg.step(k, st_g)
        _assert_transition(st_g, info_g, st_r, info_r)
        n_acc += int(info_r.is_accepted.sum())
    assert 0 < n_acc < 6 * q0.shape[0]


FUNNEL_N, FUNNEL_D = 64, 8


def _funnel_sigma(s0):
    return np.array([s0] + [0.5] * (FUNNEL_D - 1), f32)


def _funnel_restatement(s0):
    q0 = (1.5 * prng.normal(prng.key(2), (FUNNEL_N, FUNNEL_D))).astype(f32)
    fn_r = otargets.neal_funnel()
    step = rrw.normal(_funnel_sigma(s0))
    st = rrw.init(q0, fn_r)
    out = []
    for k in prng.split(prng.key(4), 5):
        st, info = rrw.additive_step_kernel(k, st, fn_r, step)
        out.append((k, st, info))
    return q0, out


@pytest.mark.parametrize("s0", [45.0, 90.0])
def test_random_walk_funnel_non_finite_proposals(dev, s0):
    """Neal's funnel with steps of 45 / 90 along its axis: proposals far down the neck have a log-density of -inf (or
    NaN) and are rejected with an acceptance rate of exactly 0 (never NaN), as safe_energy_diff prescribes; the state
    stays finite."""
    q0, ref = _funnel_restatement(s0)
    alg = bjx.normal_random_walk(bjx.targets.NealFunnel(), dev_t(_funnel_sigma(s0), dev))
    st_g = alg.init(dev_t(q0, dev))
    n_acc = n_bad = 0
    for k, st_r, info_r in ref:
        st_g, info_g = alg.step(k, st_g)
        rate = t2n(info_g.acceptance_rate)
        bad = ~np.isfinite(info_r.proposal.logdensity)
        assert np.array_equal(t2n(info_g.is_accepted), info_r.is_accepted)
        assert np.array_equal(~np.isfinite(t2n(info_g.proposal.logdensity)), bad)
        assert not np.isnan(rate).any()
        assert np.all(rate[bad] == 0) and np.all(rate[info_r.acceptance_rate == 0] == 0)
        for x in st_g:
            assert bool(torch.isfinite(x).all())
        n_acc += int(info_r.is_accepted.sum())
        n_bad += int(bad.sum())
    assert 0 < n_acc < 5 * FUNNEL_N and n_bad > 0  # the case does contain accepted, rejected and non-finite proposals


def test_random_walk_is_shard_invariant_and_chain_major(dev):
    """Chains are keyed by their GLOBAL index: chains [0, 10) and [10, 24) run with chain_offset 3 and 13 reproduce
    the unsplit run bit for bit.  A chain-major key through run_inference_algorithm equals the restatement driven
    with chain i's keys split(split(key, .)[3 + i], .)[t]."""
    N, D = 24, 64
    sig, inv_var, q0 = _gaussian_case(N, D)
    sigma = _sigma("diag", D, sig)
    fn = bjx.targets.DiagGaussian(dev_t(inv_var, dev))
    q0_g, sigma_g = dev_t(q0, dev), dev_t(sigma, dev)

    def run(lo, hi):
        alg = bjx.normal_random_walk(fn, sigma_g, chain_offset=3 + lo)
        st = alg.init(q0_g[lo:hi].contiguous())
        for k in prng.split(prng.key(9), 6):
            st, info = alg.step(k, st)
        return st, info

    def flat(st, info):
        return list(st) + [info.acceptance_rate, info.is_accepted] + list(info.proposal)

    full, a, b = flat(*run(0, N)), flat(*run(0, 10)), flat(*run(10, N))
    for f, x, y in zip(full, a, b):
        assert same_bits(f, torch.cat([x, y]))

    T = 4
    alg = bjx.normal_random_walk(fn, sigma_g, chain_offset=3)
    st_g, (hist_state, hist_info) = bjx.util.run_inference_algorithm(prng.key(21), alg, T, initial_state=alg.init(q0_g),
                                                                     key_layout="chain_major")
    assert hist_info.proposal.position.shape == (T, N, D) and hist_info.is_accepted.shape == (T, N)
    fn_r = otargets.diag_gaussian(inv_var)
    st_r = rrw.init(q0, fn_r)
    step = rrw.normal(sigma)
    chain_keys = prng.split(prng.key(21), N, offset=3)
    for t in range(T):
        st_r, info_r = rrw.additive_step_kernel(None, st_r, fn_r, step,
                                                chain_keys_override=prng.split(chain_keys, 1, offset=t)[:, 0])
        assert np.array_equal(t2n(hist_info.is_accepted[t]), info_r.is_accepted)
        np.testing.assert_allclose(t2n(hist_state.position[t]), st_r.position, rtol=1e-6, atol=1e-6)
    _assert_state(st_g, st_r)
    # and the chain-major transitions differ from the step-major ones of the same key
    st_s, _ = alg.step(prng.key(21), alg.init(q0_g))
    assert not torch.equal(st_s.position, hist_state.position[0])


def test_random_walk_plain_pytorch_logdensity_is_never_differentiated(dev):
    """A plain PyTorch function is evaluated value only -- on a tensor that does not require grad, or it raises -- and
    gives the accept bits of ``targets.DiagGaussian``."""
    N, D = 16, 64
    sig, inv_var, q0 = _gaussian_case(N, D)
    iv = dev_t(inv_var, dev)
    calls = [0]

    def logp(q):
        if q.requires_grad or torch.is_grad_enabled():
            raise AssertionError("the log-density of a gradient-free sampler was set up for differentiation")
        calls[0] += 1
        return -0.5 * (q * q * iv).sum(-1)

    sigma = float(_sigma("scalar", D, sig))
    alg_p = bjx.normal_random_walk(logp, sigma)
    alg_t = bjx.normal_random_walk(bjx.targets.DiagGaussian(iv), sigma)
    st_p, st_t = alg_p.init(dev_t(q0, dev)), alg_t.init(dev_t(q0, dev))
    n_acc = 0
    for k in prng.split(prng.key(9), 6):
        st_p, info_p = alg_p.step(k, st_p)
        st_t, info_t = alg_t.step(k, st_t)
        assert torch.equal(info_p.is_accepted, info_t.is_accepted)
        n_acc += int(info_t.is_accepted.sum())
    assert 0 < n_acc < 6 * N and calls[0] == 7  # init + one value per transition
    assert same_bits(st_p.position, st_t.position)  # the positions do not depend on how logp was summed
    np.testing.assert_allclose(t2n(st_p.logdensity), t2n(st_t.logdensity), rtol=1e-5, atol=1e-5)


def test_random_walk_outputs_are_out_of_place_and_validation(dev):
    """``step`` leaves the tensors of the state it was given untouched; ``info.proposal`` holds the proposed tensors
    themselves; argument checks; an empty batch is a no-op; a host tensor raises."""
    N, D = 24, 64
    sig, inv_var, q0 = _gaussian_case(N, D)
    fn = bjx.targets.DiagGaussian(dev_t(inv_var, dev))
    sigma_g = dev_t(_sigma("diag", D, sig), dev)
    alg = bjx.normal_random_walk(fn, sigma_g)
    st = alg.init(dev_t(q0, dev))
    before = [x.clone() for x in st]
    new, info = alg.step(prng.key(9), st)
    for x, x0, y in zip(st, before, new):
        assert same_bits(x, x0) and y.data_ptr() != x.data_ptr()
    acc = info.is_accepted
    assert bool(acc.any()) and not bool(acc.all()) and not same_bits(new.position, st.position)
    assert new.position.shape == (N, D) and new.logdensity.shape == (N,) and info.acceptance_rate.shape == (N,)
    assert same_bits(new.position[acc], info.proposal.position[acc]) and same_bits(new.position[~acc], st.position[~acc])
    assert same_bits(new.logdensity, torch.where(acc, info.proposal.logdensity, st.logdensity))
    assert info.proposal.position.data_ptr() not in (st.position.data_ptr(), new.position.data_ptr())

    # info.proposal.position IS the tensor the generator returned, info.proposal.logdensity the one the callable did
    made = {}

    def generator(rng_key, position):
        made["q1"] = position + 0.1 * bjx.random.chain_normal(rng_key, N, D, device=dev, child=0)
        return made["q1"]

    def logp(q):
        made["logp"] = fn(q)[0]
        return made["logp"]

    _, info_u = bjx.rmh(logp, generator).step(prng.key(9), st)
    assert info_u.proposal.position is made["q1"]
    assert info_u.proposal.logdensity.data_ptr() == made["logp"].data_ptr()
    # a user random_step equals the fused normal step up to the rounding of the separate product
    step = prw.normal(sigma_g)
    new_u, info_s = bjx.additive_step_random_walk(fn, lambda k, q: step(k, q)).step(prng.key(9), st)
    assert torch.equal(info_s.is_accepted, info.is_accepted)
    np.testing.assert_allclose(t2n(new_u.position), t2n(new.position), rtol=1e-6, atol=1e-6)

    with pytest.raises(ValueError):
        bjx.normal_random_walk(fn, torch.ones(D + 1, device=dev)).step(prng.key(9), st)  # (D,) of the wrong length
    with pytest.raises(NotImplementedError):
        bjx.normal_random_walk(fn, torch.ones(N, device=dev)).step(prng.key(9), st)  # one sigma per chain
    with pytest.raises(ValueError):
        bjx.normal_random_walk(fn, torch.eye(D + 1, device=dev)).step(prng.key(9), st)  # matrix of the wrong size
    with pytest.raises(ValueError):
        bjx.rmh(fn, lambda k, q: q[:, :-1]).step(prng.key(9), st)  # proposal of the wrong shape
    with pytest.raises(ValueError):
        bjx.rmh(fn, lambda k, q: q + 0.1, lambda a, b: a.position).step(prng.key(9), st)  # f must be (N,)
    with pytest.raises(ValueError):
        alg.init(torch.zeros(D, device=dev))  # not (n_chains, dim)
    with pytest.raises(RuntimeError):
        alg.init(torch.zeros(3, D))  # host tensor: there is no CPU fallback
    with pytest.raises(RuntimeError):
        bjx.irmh(fn, lambda k: torch.zeros(N, D)).step(prng.key(9), st)  # a generator that draws on the host
    e = bjx.normal_random_walk(fn, 0.1).init(torch.zeros(0, D, device=dev))
    for sigma in (0.1, sigma_g, torch.eye(D, device=dev)):
        e2, einfo = bjx.normal_random_walk(fn, sigma).step(prng.key(1), e)
        assert e2.position.shape == (0, D) and einfo.is_accepted.shape == (0,)
        assert einfo.proposal.position.shape == (0, D)

    last, (hist_state, hist_info) = bjx.util.run_inference_algorithm(prng.key(5), bjx.normal_random_walk(fn, 0.01), 3,
                                                                     initial_position=dev_t(q0, dev))
    assert hist_state.position.shape == (3, N, D) and hist_info.is_accepted.shape == (3, N)
    assert same_bits(last.position, hist_state.position[-1])


# ----------------------------------------------------------------------------- inside tempered SMC
SMC_N, SMC_D, SMC_STEPS = 64, 4, 3


def _smc_case():
    ivp = np.linspace(0.5, 2.0, SMC_D).astype(f32)
    ivl = (np.linspace(1.0, 3.0, SMC_D) * (3.5 / np.sqrt(SMC_D))).astype(f32)
    x0 = (prng.normal(prng.key(3), (SMC_N, SMC_D)) / np.sqrt(ivp)).astype(f32)
    w = np.random.default_rng(5).random(SMC_N) ** 2
    w[::7] = 0.0  # some particles are dropped, others duplicated
    return ivp, ivl, rsmc.TemperedSMCState(x0, (w / w.sum()).astype(f32), f32(0.1))


def _rw_move(sigma):
    step = rrw.normal(sigma)
    return rsmc.Move(rrw.init, lambda keys, st, fn: rrw.additive_step_kernel(None, st, fn, step,
                                                                             chain_keys_override=keys))


def _assert_smc_step(st_g, info_g, st_r, info_r):
    assert info_g.ancestors.dtype == torch.int32 and np.array_equal(t2n(info_g.ancestors), info_r.ancestors)
    assert np.array_equal(t2n(info_g.update_info.is_accepted), info_r.update_info.is_accepted)
    np.testing.assert_allclose(t2n(st_g.particles), st_r.particles, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(t2n(st_g.weights), st_r.weights, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(t2n(info_g.log_likelihood_increment), info_r.log_likelihood_increment, rtol=1e-6,
                               atol=1e-7)
    counts = np.bincount(info_r.ancestors, minlength=SMC_N)
    assert counts.max() >= 2 and counts.min() == 0
    n_acc = int(info_r.update_info.is_accepted.sum())
    assert 0 < n_acc < SMC_N


def test_random_walk_moves_tempered_smc(dev):
    """One tempered_smc step and one adaptive_tempered_smc step whose move is 3 random-walk transitions, from a state
    with uneven weights, against tests/smc_restatement.py driven by the random-walk restatement: ancestors and accept
    bits exact, particles and weights to the tolerances of test_smc_gpu.py.  The move evaluates the tempered
    log-density value only (``TemperedLogDensity._bjx_value``): the user callables are never asked for a gradient."""
    ivp, ivl, st0 = _smc_case()
    prior_r, lik_r = otargets.diag_gaussian(ivp), otargets.diag_gaussian(ivl)
    prior_g, lik_g = bjx.targets.DiagGaussian(dev_t(ivp, dev)), bjx.targets.DiagGaussian(dev_t(ivl, dev))
    params = {"random_step": prw.normal(0.5)}
    step_fn, init_fn = bjx.additive_step_random_walk.build_kernel(), bjx.additive_step_random_walk.init
    move = _rw_move(0.5)
    st0_g = smc.tempered.TemperedSMCState(dev_t(st0.particles, dev), dev_t(st0.weights, dev), dev_t(st0.lmbda, dev))

    fixed = bjx.tempered_smc(prior_g, lik_g, step_fn, init_fn, params, smc.resampling.systematic,
                             num_mcmc_steps=SMC_STEPS)
    st_g, info_g = fixed.step(prng.key(11), st0_g, 0.4)
    st_r, info_r = rsmc.tempered_step(prng.key(11), st0, f32(0.4), prior_r, lik_r, move, SMC_STEPS)
    _assert_smc_step(st_g, info_g, st_r, info_r)
    assert f32(st_g.lmbda.item()) == f32(0.4)
    assert isinstance(info_g.update_info, prw.RWInfo)

    adaptive = bjx.adaptive_tempered_smc(prior_g, lik_g, step_fn, init_fn, params, smc.resampling.systematic, 0.5,
                                         num_mcmc_steps=SMC_STEPS)
    st_g, info_g = adaptive.step(prng.key(12), st0_g)
    lam_g = f32(st_g.lmbda.item())
    _, lam_r = rsmc.next_temperature(lik_r(st0.particles)[0], 0.5, st0.lmbda)
    assert abs(float(lam_g) - float(lam_r)) <= 1e-4 * (1.0 - float(st0.lmbda)) and st0.lmbda < lam_g <= 1
    st_r, info_r = rsmc.tempered_step(prng.key(12), st0, lam_g, prior_r, lik_r, move, SMC_STEPS)
    _assert_smc_step(st_g, info_g, st_r, info_r)


def test_tempered_value_is_bit_equal_to_the_pair(dev):
    """``TemperedLogDensity._bjx_value(q)`` is the first element of ``TemperedLogDensity(q)`` bit for bit, at two
    temperatures, and is what ``_util.eval_value`` asks for."""
    from blackjax_amd._util import eval_value

    ivp, ivl, st0 = _smc_case()
    tempered = smc.tempered.TemperedLogDensity(bjx.targets.DiagGaussian(dev_t(ivp, dev)),
                                               bjx.targets.DiagGaussian(dev_t(ivl, dev)))
    q = dev_t(st0.particles, dev)
    seen = []
    for lam in (0.3, 0.85):
        tempered.set_temperature(dev_t(f32(lam), dev))
        value, pair = tempered._bjx_value(q), tempered(q)[0]
        assert value.shape == (SMC_N,) and value.dtype == torch.float32
        assert same_bits(value, pair) and same_bits(eval_value(tempered, q), pair)
        seen.append(value)
    assert not torch.equal(seen[0], seen[1])
