"""GPU parity of contour SGLD (blackjax_amd/sgmcmc/csgld.py, csrc/bjx_sgmcmc.hip: bjx_csgld_step and bjx_csgld_update,
include/bjx_hip.h "SGMCMC") against the NumPy restatement of the reference's arithmetic, tests/csgld_restatement.py."""
import numpy as np
import pytest
import torch

import blackjax_amd as bjx
import csgld_restatement as rcs
from oracle import prng
from test_sgmcmc_gpu import KEYS, SHAPES, _arg, _case, _estimators, close, dev_t, same_bits, t2n

pytestmark = pytest.mark.gpu
f32 = np.float32
csgld = bjx.sgmcmc.csgld


def _histograms(N, M, seed):
    """Random positive normalised histograms and indices in [1, M - 1]."""
    rng = np.random.default_rng(seed)
    pdf = rng.uniform(0.05, 1.0, (N, M))
    return (pdf / pdf.sum(1, keepdims=True)).astype(f32), rng.integers(1, M, N).astype(np.int32)


@pytest.mark.parametrize("M", [2, 64])
@pytest.mark.parametrize("N,D,eps_pc,T_pc", SHAPES)
def test_langevin_step_matches_restatement(dev, N, D, eps_pc, T_pc, M):
    """One launch of bjx_csgld_step, chain_offset = 3, zeta = 1 and 0.75: positions within 1e-6 (the project's
    position tolerance).  zeta = 0: the bits of bjx_sgld_step on the same inputs.  An index outside [1, M - 1] is
    clamped on read."""
    w, q0, eps, T, mbs = _case(N, D, eps_pc, T_pc)
    est_r, _ = _estimators(w, dev)
    g = est_r(q0, mbs[0])
    pdf, idx = _histograms(N, M, 7 * N + M)
    q_g, g_g, pdf_g, idx_g = (dev_t(x, dev) for x in (q0, g, pdf, idx))
    eps_g, T_g = _arg(eps, dev), _arg(T, dev)
    for zeta in (1.0, 0.75):
        got = csgld.langevin_step(KEYS[0], q_g, g_g, pdf_g, idx_g, eps_g, T_g, zeta=zeta, chain_offset=3)
        assert got.dtype == torch.float32 and got.shape == (N, D) and got.data_ptr() != q_g.data_ptr()
        close(got, rcs.langevin_step(KEYS[0], q0, g, pdf, idx, eps, T, zeta, 10.0, chain_offset=3))

    plain = bjx.sgmcmc.diffusions.overdamped_langevin()(KEYS[0], q_g, g_g, eps_g, T_g, chain_offset=3)
    zero = csgld.langevin_step(KEYS[0], q_g, g_g, pdf_g, idx_g, eps_g, T_g, zeta=0.0, chain_offset=3)
    assert same_bits(zero, plain) and not same_bits(got, plain)

    wild, tame = idx.copy(), idx.copy()
    wild[0], wild[-1] = 0, M + 5
    tame[0], tame[-1] = 1, M - 1
    out_wild = csgld.langevin_step(KEYS[0], q_g, g_g, pdf_g, dev_t(wild, dev), eps_g, T_g, zeta=0.75, chain_offset=3)
    out_tame = csgld.langevin_step(KEYS[0], q_g, g_g, pdf_g, dev_t(tame, dev), eps_g, T_g, zeta=0.75, chain_offset=3)
    assert same_bits(out_wild, out_tame)
    close(out_wild, rcs.langevin_step(KEYS[0], q0, g, pdf, tame, eps, T, 0.75, 10.0, chain_offset=3))


GAP, MIN_E = 8.0, -16.0


def _logdensities(N, M):
    """(calls, N) log-densities holding: an energy below min_energy; one beyond the last bin; the exact bin edges
    -(min_energy + k gap), k = 0 .. M (exact in fp32: the gap is a power of two) and their fp32 neighbours on both
    sides; NaN, +inf and -inf; padded with random energies over the whole range."""
    edges = MIN_E + GAP * np.arange(M + 1, dtype=np.float64)
    edges = edges[np.unique(np.clip([0, 1, 2, 3, M // 2, M - 3, M - 2, M - 1, M], 0, M))].astype(f32)
    energies = np.concatenate([f32([MIN_E - 100.0, MIN_E + GAP * M + 1000.0, np.nan, np.inf, -np.inf]), edges,
                               np.nextafter(edges, f32(-np.inf)), np.nextafter(edges, f32(np.inf))]).astype(f32)
    calls = -(-len(energies) // N)
    rng = np.random.default_rng(M)
    pad = rng.uniform(MIN_E - GAP, MIN_E + GAP * (M + 1), calls * N - len(energies)).astype(f32)
    return (-np.concatenate([energies, pad])).astype(f32).reshape(calls, N)


@pytest.mark.parametrize("N,M", [(5, 2), (37, 3), (16, 64), (7, 65), (33, 512), (3, 513), (9, 2052)])
def test_update_energy_histogram_matches_restatement(dev, N, M):
    """One launch of bjx_csgld_update with energy_gap = 8, min_energy = -16, scalar and per-chain step_size_stoch.
    zeta = 1: equal indices, histograms with the same bits.  zeta = 0.75: equal indices, every entry within
    2^-23 w |u_j| + 2 ulp of the restatement (the device pow, rounded once from fp64, can differ from NumPy's by one
    fp32 ulp of w)."""
    pdf, _ = _histograms(N, M, 11 * N + M)
    pdf_g = dev_t(pdf, dev)
    eps_pc = (f32(0.05) * np.random.default_rng(N).uniform(0.5, 1.5, N)).astype(f32)
    seen = set()
    for ld in _logdensities(N, M):
        ld_g = dev_t(ld, dev)
        for eps in (0.05, eps_pc):
            for zeta in (1.0, 0.75):
                new_pdf, new_idx = csgld.update_energy_histogram(ld_g, pdf_g, _arg(eps, dev), zeta=zeta,
                                                                 energy_gap=GAP, min_energy=MIN_E)
                ref_pdf, ref_idx = rcs.update_energy_histogram(ld, pdf, eps, zeta, GAP, MIN_E)
                assert new_pdf.dtype == torch.float32 and new_pdf.shape == (N, M)
                assert new_idx.dtype == torch.int32 and np.array_equal(t2n(new_idx), ref_idx)
                if zeta == 1.0:
                    assert np.array_equal(t2n(new_pdf).view(np.uint32), ref_pdf.view(np.uint32))
                else:
                    rows = np.arange(N)
                    u = -pdf.astype(np.float64)
                    u[rows, ref_idx] += 1.0
                    a = pdf[rows, ref_idx].astype(np.float64)
                    w = np.broadcast_to(np.asarray(eps, np.float64), (N,)) * a ** zeta
                    tol = 2.0 ** -23 * w[:, None] * np.abs(u) + 2.0 * np.spacing(np.abs(ref_pdf)).astype(np.float64)
                    err = np.abs(t2n(new_pdf).astype(np.float64) - ref_pdf.astype(np.float64))
                    print("zeta 0.75: largest error / tolerance", float((err / tol).max()))
                    assert np.all(err <= tol)
        seen.update(ref_idx.tolist())
        assert ref_idx[np.isnan(ld)].tolist() == [1] * int(np.isnan(ld).sum())
        assert np.all(ref_idx[ld == np.inf] == 1) and np.all(ref_idx[ld == -np.inf] == M - 1)
    assert {1, M - 1} <= seen and (M < 4 or len(seen) >= 4)


def _double_well(dev):
    """The device estimators of csgld_restatement's double well; the minibatch is the 0-d device tensor c."""
    def logdensity(q, c):
        return -((q * q).sum(-1) - c) ** 2 / 8.0

    def gradient(q, c):
        return -(((q * q).sum(-1) - c) / 2.0)[:, None] * q

    return logdensity, gradient


@pytest.mark.parametrize("D", [10, 260])
def test_csgld_steps_match_restatement(dev, D):
    """init + six consecutive steps without re-sync on the double well, N = 33, M = 64, zeta = 0.75, chain_offset = 3.
    The restatement floors the log-densities the device estimator returned at that step, so both sides floor the same
    fp32 numbers.  Per step: positions within 1e-6, equal indices, histograms within 1e-6.  Each estimator is called
    once per step, the gradient's at the old position and the log-density's at the very position the step returns."""
    N, M, zeta = 33, 64, 0.75
    q0, eps, eps_sa, T, mbs, gap, min_e = rcs.double_well_case(N, D)
    logdensity, gradient = _double_well(dev)
    calls = []

    def logdensity_recorded(q, c):
        calls.append(("logdensity", q, logdensity(q, c)))
        return calls[-1][2]

    def gradient_recorded(q, c):
        calls.append(("gradient", q, None))
        return gradient(q, c)

    alg = bjx.csgld(logdensity_recorded, gradient_recorded, zeta, M, gap, min_e, chain_offset=3)
    st_g, st_r = alg.init(dev_t(q0, dev)), rcs.init(q0, M)
    assert isinstance(st_g, csgld.ContourSGLDState) and st_g.energy_idx.dtype == torch.int32
    assert np.array_equal(t2n(st_g.energy_pdf).view(np.uint32), st_r.energy_pdf.view(np.uint32))
    assert np.array_equal(t2n(st_g.energy_idx), st_r.energy_idx)
    history = []
    for k, m in zip(KEYS, mbs):
        calls.clear()
        old = st_g
        st_g = alg.step(k, st_g, dev_t(m, dev), _arg(eps, dev), _arg(eps_sa, dev), _arg(T, dev))
        assert [c[0] for c in calls] == ["gradient", "logdensity"]
        assert calls[0][1].data_ptr() == old.position.data_ptr() and calls[1][1] is st_g.position
        replay = t2n(calls[1][2])
        st_r = rcs.csgld_kernel(k, st_r, lambda q, mb: replay, rcs.double_well_gradient_estimator, m, eps, eps_sa,
                                zeta, T, gap, min_e, chain_offset=3)
        close(st_g.position, st_r.position)
        assert np.array_equal(t2n(st_g.energy_idx), st_r.energy_idx)
        close(st_g.energy_pdf, st_r.energy_pdf)
        history.append(st_r.energy_idx)
    assert len(np.unique(np.concatenate(history))) >= 3  # or the index path is not exercised
    assert not np.allclose(st_r.position, q0)


def _bincount(history, M):
    """(T, N) device index history -> (N, M) counts, by torch.bincount."""
    T, N = history.shape
    flat = (torch.arange(N, device=history.device)[None] * M + history.long()).flatten()
    return torch.bincount(flat, minlength=N * M).view(N, M)


def test_csgld_with_zeta_zero_is_sgld_and_a_running_histogram(dev):
    """zeta = 0, T = 32, N = 33, D = 10, M = 65.  The update is then pdf <- pdf + step_size_stoch (e_i - pdf), a
    running mean of the visited bins, and the position path is sgld's.

    With step_size_stoch = 1 / (t + 1) the first update (weight 1) empties every bin but one, and the next multiplier
    is 0 * (log 0 - log 0) = NaN, in the reference as here (a non-positive histogram entry gives a NaN row), so that
    schedule cannot be held against ``sgld`` beyond its first step.  Hence two runs.

    * 1 / (t + 2), which keeps init's row as one observation and every bin positive: through all 32 steps on the
      double well the positions have the same bits as ``blackjax_amd.sgld`` run with the same keys, and the histogram
      is (init's row + torch.bincount of the index history) / (T + 1) within 4 T 2^-24.
    * 1 / (t + 1), the log-density estimator returning a prescribed energy sequence (the minibatch): the histogram is
      torch.bincount of the index history / T within 4 T 2^-24; the first step has sgld's bits and the positions are
      NaN from the second on.
    """
    N, D, M, T = 33, 10, 65, 32
    q0, eps, _, temp, _, gap, min_e = rcs.double_well_case(N, D)
    logdensity, gradient = _double_well(dev)
    keys = prng.split(prng.key(13), T)
    eps_g, temp_g = _arg(eps, dev), _arg(temp, dev)
    tol = 4 * T * 2.0 ** -24

    alg, sgld = bjx.csgld(logdensity, gradient, 0, M, gap, min_e, chain_offset=3), bjx.sgld(gradient, chain_offset=3)
    st = alg.init(dev_t(q0, dev))
    row0, q, history = st.energy_pdf.double(), sgld.init(dev_t(q0, dev)), []
    for t, k in enumerate(keys):
        c = torch.tensor(4.0 + 0.5 * np.sin(1.0 + t), dtype=torch.float32, device=dev)
        st = alg.step(k, st, c, eps_g, 1.0 / (t + 2), temp_g)
        q = sgld.step(k, q, c, eps_g, temp_g)
        assert same_bits(st.position, q)
        history.append(st.energy_idx)
    history = torch.stack(history)
    assert len(torch.unique(history)) >= 3
    expect = (row0 + _bincount(history, M).double()) / (T + 1)
    err = float((st.energy_pdf.double() - expect).abs().max())
    print("1 / (t + 2): largest histogram error", err, "bound", tol)
    assert err <= tol

    rng = np.random.default_rng(4)
    alg = bjx.csgld(lambda q, energies: -energies, gradient, 0, M, 10.0, 0.0, chain_offset=3)
    st, history = alg.init(dev_t(q0, dev)), []
    for t, k in enumerate(keys):
        energies = dev_t(rng.uniform(-20.0, 700.0, N).astype(f32), dev)
        st = alg.step(k, st, energies, eps_g, 1.0 / (t + 1), temp_g)
        if t == 0:
            assert same_bits(st.position, sgld.step(k, dev_t(q0, dev), energies, eps_g, temp_g))
        history.append(st.energy_idx)
    history = torch.stack(history)
    assert len(torch.unique(history)) > 30 and bool(torch.isnan(st.position).all())
    err = float((st.energy_pdf.double() - _bincount(history, M).double() / T).abs().max())
    print("1 / (t + 1): largest histogram error", err, "bound", tol)
    assert err <= tol


def test_csgld_is_shard_invariant(dev):
    """Chains are keyed by their GLOBAL index: chains [0, 10) and [10, 24) run with chain_offset 3 and 13 reproduce
    the unsplit run bit for bit, in position, histogram and index.  The estimators are element-wise (the gradient of
    test_sgmcmc_gpu.py; the log-density reads one column), so that nothing of them depends on the batch's size."""
    N, D, M = 24, 64, 64
    w, q0, eps, T, mbs = _case(N, D, True, True)
    _, est_g = _estimators(w, dev)
    q0_g, eps_g, T_g = dev_t(q0, dev), dev_t(eps, dev), dev_t(T, dev)
    eps_sa = torch.linspace(0.05, 0.15, N, device=dev)

    def logdensity(q, m):
        return -4.0 * (q[:, 0] * q[:, 0])

    def run(lo, hi):
        alg = bjx.csgld(logdensity, est_g, 0.75, M, 0.25, 0.0, chain_offset=3 + lo)
        st = alg.init(q0_g[lo:hi].contiguous())
        for t in range(4):
            st = alg.step(KEYS[t], st, dev_t(mbs[t], dev), eps_g[lo:hi].contiguous(), eps_sa[lo:hi].contiguous(),
                          T_g[lo:hi].contiguous())
        return st

    full, a, b = run(0, N), run(0, 10), run(10, N)
    assert len(torch.unique(full.energy_idx)) >= 3
    for f, x, y in zip(full, a, b):
        assert same_bits(f, torch.cat([x, y]))


def test_csgld_outputs_are_out_of_place_and_edge_sizes(dev):
    """``step`` leaves the state it was given untouched; an empty batch gives an empty state of the right shapes; a
    position and a histogram 4 bytes off 16-byte alignment (the 4-byte sweeps) give the bits of aligned copies;
    N = 1, D = 1, M = 2 runs."""
    N, D, M = 24, 64, 64
    q0, eps, eps_sa, T, mbs, gap, min_e = rcs.double_well_case(N, D)
    logdensity, gradient = _double_well(dev)
    alg = bjx.csgld(logdensity, gradient, 0.75, M, gap, min_e)
    c, k = dev_t(mbs[0], dev), KEYS[0]
    args = (_arg(eps, dev), _arg(eps_sa, dev), _arg(T, dev))
    st = alg.step(KEYS[1], alg.init(dev_t(q0, dev)), c, *args)  # a state whose rows differ
    before = [x.clone() for x in st]
    new = alg.step(k, st, c, *args)
    for x, x0, y in zip(st, before, new):
        assert same_bits(x, x0) and y.data_ptr() != x.data_ptr()
    assert not same_bits(new.position, st.position) and not same_bits(new.energy_pdf, st.energy_pdf)

    e_st = alg.step(k, alg.init(torch.zeros(0, D, device=dev)), c, 0.01, 0.1)
    assert e_st.position.shape == (0, D) and e_st.energy_pdf.shape == (0, M) and e_st.energy_idx.shape == (0,)
    assert e_st.energy_idx.dtype == torch.int32

    def odd(x):  # contiguous, 4-byte aligned, not 16-byte aligned
        buf = torch.zeros(x.numel() + 4, device=dev)
        v = buf[1:1 + x.numel()].view(x.shape)
        v.copy_(x)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v

    new_odd = alg.step(k, csgld.ContourSGLDState(odd(st.position), odd(st.energy_pdf), st.energy_idx), c, *args)
    for x, y in zip(new_odd, new):
        assert same_bits(x, y)

    tiny = bjx.csgld(logdensity, gradient, 0.75, 2, gap, min_e)
    t_st = tiny.step(k, tiny.init(torch.full((1, 1), 0.5, device=dev)), c, 0.01, 0.1)
    assert t_st.position.shape == (1, 1) and t_st.energy_pdf.shape == (1, 2) and t2n(t_st.energy_idx).tolist() == [1]
    assert bool(torch.isfinite(t_st.position).all()) and bool(torch.isfinite(t_st.energy_pdf).all())
