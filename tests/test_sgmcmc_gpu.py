"""GPU parity of the stochastic-gradient samplers (blackjax_amd/sgmcmc/, csrc/bjx_sgmcmc.hip, include/bjx_hip.h
"SGMCMC") against the NumPy restatement of the reference's arithmetic, tests/sgmcmc_restatement.py."""
import numpy as np
import pytest
import torch

import blackjax_amd as bjx
import sgmcmc_restatement as rsg
from oracle import prng

pytestmark = pytest.mark.gpu
f32 = np.float32
ALPHA = 0.05  # friction of the parity cases (the default 0.01 makes the noise a fifth of this)

# (N, D, per-chain eps, per-chain T): 4-byte sweep; one element; 16-byte sweep (scalar / per-chain); rows beyond one
# 256-float span on the 16-byte and the 4-byte sweep; the 16-byte sweep at four full spans and with a ragged last span
SHAPES = [(37, 10, True, True), (5, 1, False, False), (16, 64, False, True), (24, 64, True, False),
          (33, 260, True, True), (7, 259, True, False), (9, 1024, False, True), (3, 2052, True, True)]


def t2n(t):
    return t.detach().cpu().numpy()


def dev_t(a, dev):
    return torch.as_tensor(np.asarray(a), device=dev)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def close(a, b):
    np.testing.assert_allclose(t2n(a) if isinstance(a, torch.Tensor) else a, b, rtol=1e-6, atol=1e-6)


def _case(N, D, eps_pc, T_pc):
    """The parity cases: estimator g = (m - q) * w, a subtraction then a multiplication (nothing can contract into an
    fma, so both sides compute the same bits), w_j = 10^(1 - 2 j / (D - 1)); the minibatch IS m, (D,), fresh every
    step; q0 = normal(key(1)); eps = 0.05 and T = 1.5, times uniform(0.6, 1.6) / uniform(0.4, 1.6) per chain."""
    w = (10.0 ** (1.0 - 2.0 * np.arange(D) / max(D - 1, 1))).astype(f32)
    q0 = prng.normal(prng.key(1), (N, D))
    rng = np.random.default_rng(100 * N + D)
    eps = (f32(0.05) * rng.uniform(0.6, 1.6, N)).astype(f32) if eps_pc else 0.05
    T = (f32(1.5) * rng.uniform(0.4, 1.6, N)).astype(f32) if T_pc else 1.5
    minibatches = [prng.normal(prng.key(50 + t), (D,)) for t in range(6)]
    return w, q0, eps, T, minibatches


def _estimators(w, dev):
    w_g = dev_t(w, dev)

    def est_r(q, m):
        return ((m - q).astype(f32) * w).astype(f32)

    def est_g(q, m):
        return (m - q) * w_g

    return est_r, est_g


def _arg(x, dev):
    return dev_t(x, dev) if isinstance(x, np.ndarray) else float(x)


KEYS = prng.split(prng.key(9), 6)


@pytest.mark.parametrize("N,D,eps_pc,T_pc", SHAPES)
def test_sgld_matches_restatement(dev, N, D, eps_pc, T_pc):
    """6 consecutive steps without re-sync, chain_offset = 3: positions within 1e-6 (test_mala_gpu.py's tolerance)."""
    w, q0, eps, T, mbs = _case(N, D, eps_pc, T_pc)
    est_r, est_g = _estimators(w, dev)
    alg = bjx.sgld(est_g, chain_offset=3)
    q_g, q_r = alg.init(dev_t(q0, dev)), q0
    for k, m in zip(KEYS, mbs):
        q_r = rsg.sgld_kernel(k, q_r, est_r, m, eps, T, chain_offset=3)
        q_g = alg.step(k, q_g, dev_t(m, dev), _arg(eps, dev), _arg(T, dev))
        assert q_g.dtype == torch.float32 and q_g.shape == (N, D)
        close(q_g, q_r)
    assert not np.allclose(q_r, q0)


@pytest.mark.parametrize("L", [1, 2, 5])
@pytest.mark.parametrize("N,D,eps_pc,T_pc", SHAPES)
def test_sghmc_matches_restatement(dev, N, D, eps_pc, T_pc, L):
    """The same for sghmc; L = 1 and L = 2 are the drawn-momentum and position-only launches with no middle step.  The
    restatement evaluates all L steps, the engine L - 1 gradients."""
    w, q0, eps, T, mbs = _case(N, D, eps_pc, T_pc)
    est_r, est_g = _estimators(w, dev)
    alg = bjx.sghmc(est_g, L, alpha=ALPHA, chain_offset=3)
    q_g, q_r = alg.init(dev_t(q0, dev)), q0
    for k, m in zip(KEYS, mbs):
        q_r = rsg.sghmc_kernel(k, q_r, est_r, m, eps, L, T, alpha=ALPHA, chain_offset=3)
        q_g = alg.step(k, q_g, dev_t(m, dev), _arg(eps, dev), _arg(T, dev))
        close(q_g, q_r)
    assert not np.allclose(q_r, q0)


@pytest.mark.parametrize("N,D,eps_pc,T_pc", SHAPES)
def test_sghmc_momentum_of_a_middle_step_matches_restatement(dev, N, D, eps_pc, T_pc):
    """The momentum the sampler drops, read through the diffusion itself: two steps of ``diffusions.sghmc`` (the first
    draws the refresh) against the restatement run with L = 2 and its momentum kept."""
    w, q0, eps, T, mbs = _case(N, D, eps_pc, T_pc)
    est_r, est_g = _estimators(w, dev)
    one_step = bjx.sgmcmc.diffusions.sghmc(ALPHA, 0.0)
    q_r, p_r = rsg.sghmc_kernel(KEYS[0], q0, est_r, mbs[0], eps, 2, T, alpha=ALPHA, chain_offset=3,
                                return_momentum=True)
    q, m = dev_t(q0, dev), dev_t(mbs[0], dev)
    q, p = one_step(KEYS[0], q, None, est_g(q, m), _arg(eps, dev), _arg(T, dev), chain_offset=3, step_index=0)
    q, p = one_step(KEYS[0], q, p, est_g(q, m), _arg(eps, dev), _arg(T, dev), chain_offset=3, step_index=1)
    close(q, q_r)
    close(p, p_r)


@pytest.mark.parametrize("N,D,eps_pc,T_pc", SHAPES)
def test_sgnht_matches_restatement(dev, N, D, eps_pc, T_pc):
    """init (the momentum draw) + 6 consecutive steps: positions, momenta and xi within 1e-6."""
    w, q0, eps, T, mbs = _case(N, D, eps_pc, T_pc)
    est_r, est_g = _estimators(w, dev)
    alg = bjx.sgnht(est_g, alpha=ALPHA, chain_offset=3)
    st_g = alg.init(dev_t(q0, dev), prng.key(4))
    st_r = rsg.sgnht_init(q0, prng.key(4), ALPHA, chain_offset=3)
    assert isinstance(st_g, bjx.sgmcmc.sgnht.SGNHTState) and st_g.xi.shape == (N,)
    for a, b in zip(st_g, st_r):
        close(a, b)
    for k, m in zip(KEYS, mbs):
        st_r = rsg.sgnht_kernel(k, st_r, est_r, m, eps, T, alpha=ALPHA, chain_offset=3)
        st_g = alg.step(k, st_g, dev_t(m, dev), _arg(eps, dev), _arg(T, dev))
        for a, b in zip(st_g, st_r):
            close(a, b)
    assert not np.allclose(st_r.xi, ALPHA)
    xi0 = np.linspace(0.0, 0.3, N).astype(f32)  # init with a per-chain xi
    st = bjx.sgnht.init(dev_t(q0, dev), prng.key(4), dev_t(xi0, dev), chain_offset=3)
    assert np.array_equal(t2n(st.xi), xi0) and same_bits(st.momentum, alg.init(dev_t(q0, dev), prng.key(4)).momentum)


def test_sghmc_calls_the_estimator_once_less_than_it_integrates(dev):
    N, D = 16, 64
    w, q0, eps, T, mbs = _case(N, D, False, False)
    _, est_g = _estimators(w, dev)
    calls = []

    def counted(q, m):
        calls.append(1)
        return est_g(q, m)

    for L in (1, 2, 5):
        calls.clear()
        bjx.sghmc(counted, L).step(KEYS[0], dev_t(q0, dev), dev_t(mbs[0], dev), eps)
        assert len(calls) == L - 1


def _runners(dev, N, D):
    """name -> run(lo, hi, key_of_step) of chains [lo, hi) with chain_offset 3 + lo over 4 steps -> tuple of tensors."""
    w, q0, eps, T, mbs = _case(N, D, True, True)
    _, est_g = _estimators(w, dev)
    q0_g, eps_g, T_g = dev_t(q0, dev), dev_t(eps, dev), dev_t(T, dev)

    def sl(x, lo, hi):
        return x[lo:hi].contiguous()

    def sgld(lo, hi, key_of):
        alg, q = bjx.sgld(est_g, chain_offset=3 + lo), sl(q0_g, lo, hi)
        for t in range(4):
            q = alg.step(key_of(t), q, dev_t(mbs[t], dev), sl(eps_g, lo, hi), sl(T_g, lo, hi))
        return (q,)

    def sghmc(lo, hi, key_of):
        alg, q = bjx.sghmc(est_g, 3, alpha=ALPHA, chain_offset=3 + lo), sl(q0_g, lo, hi)
        for t in range(4):
            q = alg.step(key_of(t), q, dev_t(mbs[t], dev), sl(eps_g, lo, hi), sl(T_g, lo, hi))
        return (q,)

    def sgnht(lo, hi, key_of):
        alg = bjx.sgnht(est_g, alpha=ALPHA, chain_offset=3 + lo)
        st = alg.init(sl(q0_g, lo, hi), prng.key(4))
        for t in range(4):
            st = alg.step(key_of(t), st, dev_t(mbs[t], dev), sl(eps_g, lo, hi), sl(T_g, lo, hi))
        return tuple(st)

    return {"sgld": sgld, "sghmc": sghmc, "sgnht": sgnht}


@pytest.mark.parametrize("name", ["sgld", "sghmc", "sgnht"])
def test_sgmcmc_is_shard_invariant_and_chain_major(dev, name):
    """Chains are keyed by their GLOBAL index: chains [0, 10) and [10, 24) run with chain_offset 3 and 13 reproduce the
    unsplit run bit for bit.  A ``ChainMajorKey`` step equals the restatement driven with chain i's keys
    split(split(key, .)[3 + i], .)[t], and differs from the step-major step of the same key."""
    N, D = 24, 64
    run = _runners(dev, N, D)[name]
    full, a, b = run(0, N, lambda t: KEYS[t]), run(0, 10, lambda t: KEYS[t]), run(10, N, lambda t: KEYS[t])
    for f, x, y in zip(full, a, b):
        assert same_bits(f, torch.cat([x, y]))

    w, q0, eps, T, mbs = _case(N, D, True, True)
    est_r, _ = _estimators(w, dev)
    major = run(0, N, lambda t: bjx.random.ChainMajorKey(prng.key(21), t))
    chain_keys = prng.split(prng.key(21), N, offset=3)
    over = [prng.split(chain_keys, 1, offset=t)[:, 0] for t in range(4)]
    if name == "sgnht":
        # init draws the momentum with the plain key(4) in both runs
        st = rsg.sgnht_init(q0, prng.key(4), ALPHA, chain_offset=3)
        for t in range(4):
            st = rsg.sgnht_kernel(None, st, est_r, mbs[t], eps, T, alpha=ALPHA, chain_keys_override=over[t])
        expect = tuple(st)
    else:
        q = q0
        for t in range(4):
            if name == "sgld":
                q = rsg.sgld_kernel(None, q, est_r, mbs[t], eps, T, chain_keys_override=over[t])
            else:
                q = rsg.sghmc_kernel(None, q, est_r, mbs[t], eps, 3, T, alpha=ALPHA, chain_keys_override=over[t])
        expect = (q,)
    for x, y in zip(major, expect):
        close(x, y)
    step_major = run(0, N, lambda t: prng.key(21))
    assert not torch.equal(step_major[0], major[0])


def test_sgmcmc_outputs_are_out_of_place_and_edge_sizes(dev):
    """``step`` leaves the tensors it was given untouched; an empty batch is a no-op; a row block at an address that is
    4- but not 16-byte aligned takes the 4-byte sweep and still matches the restatement."""
    N, D = 24, 64
    w, q0, eps, T, mbs = _case(N, D, True, True)
    est_r, est_g = _estimators(w, dev)
    eps_g, T_g, m_g, k = dev_t(eps, dev), dev_t(T, dev), dev_t(mbs[0], dev), KEYS[0]
    sgld, sghmc, sgnht = bjx.sgld(est_g), bjx.sghmc(est_g, 3, alpha=ALPHA), bjx.sgnht(est_g, alpha=ALPHA)

    q = dev_t(q0, dev)
    for alg in (sgld, sghmc):
        before = q.clone()
        new = alg.step(k, q, m_g, eps_g, T_g)
        assert same_bits(q, before) and new.data_ptr() != q.data_ptr() and not same_bits(new, q)
    st = sgnht.init(q, prng.key(4))
    before = [x.clone() for x in st]
    new = sgnht.step(k, st, m_g, eps_g, T_g)
    for x, x0, y in zip(st, before, new):
        assert same_bits(x, x0) and y.data_ptr() != x.data_ptr() and not same_bits(y, x)

    with pytest.raises(ValueError):
        sgld.step(k, q, m_g, torch.ones(N + 1, device=dev))  # per-chain step size of the wrong length
    with pytest.raises(ValueError):
        sgld.step(k, q, m_g, 0.1, torch.ones(N - 1, device=dev))  # per-chain temperature of the wrong length

    e = torch.zeros(0, D, device=dev)
    assert sgld.step(k, e, m_g, 0.1).shape == (0, D) and sghmc.step(k, e, m_g, 0.1).shape == (0, D)
    e_st = sgnht.step(k, sgnht.init(e, prng.key(4)), m_g, 0.1)
    assert e_st.position.shape == (0, D) and e_st.momentum.shape == (0, D) and e_st.xi.shape == (0,)

    # 16-byte rows (D = 64) at an odd float offset: contiguous, 4-byte aligned, not 16-byte aligned
    buf = torch.zeros(N * D + 4, device=dev)
    q_odd = buf[1:1 + N * D].view(N, D)
    q_odd.copy_(q)
    assert q_odd.is_contiguous() and q_odd.data_ptr() % 16 == 4
    close(sgld.step(k, q_odd, m_g, eps_g, T_g), rsg.sgld_kernel(k, q0, est_r, mbs[0], eps, T))
    close(sghmc.step(k, q_odd, m_g, eps_g, T_g), rsg.sghmc_kernel(k, q0, est_r, mbs[0], eps, 3, T, alpha=ALPHA))
    st_odd = sgnht.step(k, sgnht.init(q_odd, prng.key(4)), m_g, eps_g, T_g)
    st_r = rsg.sgnht_kernel(k, rsg.sgnht_init(q0, prng.key(4), ALPHA), est_r, mbs[0], eps, T, alpha=ALPHA)
    for a, b in zip(st_odd, st_r):
        close(a, b)


# ---- the samplers as samplers, on the device (shapes, expected values and margin of tests/test_sgmcmc_api.py) --------
N_STAT, D_STAT = 4096, 8
SE_REL = np.sqrt(2.0 / (N_STAT * D_STAT))


def exact_gradient(q, minibatch):
    return -q


@pytest.mark.parametrize("T", [1.0, 2.0])
def test_sgld_device_stationary_variance(dev, T):
    """Target N(0, 1), g = -q, eps = 0.5, 30 steps from q = 0: pooled variance within 5 s.e. of T / (1 - eps / 2)."""
    eps = 0.5
    alg = bjx.sgld(exact_gradient)
    q = torch.zeros(N_STAT, D_STAT, device=dev)
    for k in prng.split(prng.key(31), 30):
        q = alg.step(k, q, None, eps, T)
    var, expected = float(q.double().var(unbiased=False)), T / (1.0 - eps / 2.0)
    print("sgld pooled variance", var, "expected", expected, "s.e.", abs(var / expected - 1.0) / SE_REL)
    assert abs(var / expected - 1.0) <= 5.0 * SE_REL


@pytest.mark.parametrize("T", [1.0, 2.0])
def test_sghmc_device_stationary_variance(dev, T):
    """eps = 0.3, alpha = 0.3, beta = 0, L = 5, 12 kernel calls: pooled variance within 5 s.e. of the fixed point of
    the restated linear recursion (1.43537 at T = 1, 1.80198 at T = 2)."""
    eps, alpha, beta, L = 0.3, 0.3, 0.0, 5
    expected, _ = rsg.sghmc_stationary_variance(eps, alpha, beta, L, T)
    alg = bjx.sghmc(exact_gradient, L, alpha, beta)
    q = torch.zeros(N_STAT, D_STAT, device=dev)
    for k in prng.split(prng.key(32), 12):
        q = alg.step(k, q, None, eps, T)
    var = float(q.double().var(unbiased=False))
    print("sghmc pooled variance", var, "expected", expected, "s.e.", abs(var / expected - 1.0) / SE_REL)
    assert abs(var / expected - 1.0) <= 5.0 * SE_REL


def test_sgld_end_to_end_gaussian_mean_posterior(dev):
    """``gradients.grad_estimator`` (autograd) on the Gaussian-mean model -- prior N(0, I), M = 512 data y_b ~ N(q, I),
    minibatches of B = 32 drawn afresh for every chain and step, so the chains are independent -- drives ``sgld`` for
    200 steps at eps = 1e-3 (eps x posterior precision = 0.513).  The drift is linear and the estimator unbiased, so
    the chain mean converges to the conjugate posterior mean sum(y) / (1 + M) exactly; the pooled mean of the 4 096
    chains is within 5 s.e. of it in every dimension, the s.e. taken from the restatement run of the same
    configuration (its per-dimension standard deviation over chains / sqrt(N))."""
    N, D, M, B, steps, eps = 4096, 8, 512, 32, 200, 1e-3
    y = (f32(1.0) + prng.normal(prng.key(7), (M, D))).astype(f32)
    posterior_mean = y.astype(np.float64).sum(0) / (1.0 + M)
    rng = np.random.default_rng(5)

    def logprior_fn(q):
        return -0.5 * (q * q).sum(-1)

    def loglikelihood_fn(q, minibatch):  # (N, D), (N, B, D) -> (N, B)
        return -0.5 * ((minibatch - q[:, None, :]) ** 2).sum(-1)

    alg = bjx.sgld(bjx.sgmcmc.grad_estimator(logprior_fn, loglikelihood_fn, M))
    est_r = rsg.gaussian_mean_grad_estimator(1.0, M)
    y_g = dev_t(y, dev)
    q_g, q_r = alg.init(torch.zeros(N, D, device=dev)), np.zeros((N, D), f32)
    for k in prng.split(prng.key(8), steps):
        idx = rng.integers(0, M, (N, B))
        q_r = rsg.sgld_kernel(k, q_r, est_r, y[idx], eps)
        q_g = alg.step(k, q_g, y_g[dev_t(idx, dev)], eps)
    se = q_r.astype(np.float64).std(0, ddof=1) / np.sqrt(N)
    dev_mean, r_mean = t2n(q_g).astype(np.float64).mean(0), q_r.astype(np.float64).mean(0)
    print("posterior mean", posterior_mean, "\ndevice (s.e.)", np.abs(dev_mean - posterior_mean) / se,
          "\nrestatement (s.e.)", np.abs(r_mean - posterior_mean) / se, "\nchain sd", se * np.sqrt(N),
          "posterior sd", (1.0 + M) ** -0.5)
    assert np.all(np.abs(dev_mean - posterior_mean) <= 5.0 * se)
    assert np.all(np.abs(r_mean - posterior_mean) <= 5.0 * se)
