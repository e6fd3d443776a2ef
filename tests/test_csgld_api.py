"""``blackjax_amd.csgld``: API surface, the two C entry points' argument checks and the Python argument errors (no GPU
needed), and the NumPy restatement the GPU tests hold the kernels against (tests/csgld_restatement.py), checked on its
own."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import csgld_restatement as rcs
import sgmcmc_restatement as rsg
from oracle import prng

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def exact_gradient(q, minibatch):
    return -q


def exact_logdensity(q, minibatch):
    return -0.5 * (q * q).sum(-1)


def _params(fn):
    return [(p.name, p.kind, p.default) for p in inspect.signature(fn).parameters.values()]


def test_csgld_exports_and_signatures():
    import blackjax_amd as bjx
    from blackjax_amd import _lib

    P, K, E = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.empty
    mod = bjx.sgmcmc.csgld
    assert "csgld" in bjx.__all__ and "csgld" in bjx.sgmcmc.__all__ and inspect.ismodule(mod)
    assert isinstance(bjx.csgld, bjx.GenerateSamplingAPI)
    assert bjx.csgld.init is mod.init and bjx.csgld.build_kernel is mod.build_kernel
    assert bjx.csgld.differentiable is mod.as_top_level_api
    assert mod.ContourSGLDState._fields == rcs.ContourSGLDState._fields == ("position", "energy_pdf", "energy_idx")

    assert _params(mod.init) == [("position", P, E), ("num_partitions", P, 512)]
    assert _params(mod.build_kernel) == [("num_partitions", P, 512), ("energy_gap", P, 10), ("min_energy", P, 0)]
    assert _params(mod.build_kernel()) == [
        ("rng_key", P, E), ("state", P, E), ("logdensity_estimator", P, E), ("gradient_estimator", P, E),
        ("minibatch", P, E), ("step_size_diff", P, E), ("step_size_stoch", P, E), ("zeta", P, 1),
        ("temperature", P, 1.0), ("chain_offset", K, 0)]
    assert _params(mod.as_top_level_api) == [
        ("logdensity_estimator", P, E), ("gradient_estimator", P, E), ("zeta", P, 1), ("num_partitions", P, 512),
        ("energy_gap", P, 100), ("min_energy", P, 0), ("chain_offset", K, 0)]
    assert _params(mod.langevin_step) == [
        ("rng_key", P, E), ("position", P, E), ("logdensity_grad", P, E), ("energy_pdf", P, E), ("energy_idx", P, E),
        ("step_size_diff", P, E), ("temperature", P, 1.0), ("zeta", K, 1.0), ("energy_gap", K, 10.0),
        ("chain_offset", K, 0)]
    assert _params(mod.update_energy_histogram) == [
        ("logdensity", P, E), ("energy_pdf", P, E), ("step_size_stoch", P, E), ("zeta", K, 1.0),
        ("energy_gap", K, 10.0), ("min_energy", K, 0.0)]

    alg = bjx.csgld(exact_logdensity, exact_gradient)
    assert isinstance(alg, bjx.SamplingAlgorithm)
    assert _params(alg.init) == [("position", P, E), ("rng_key", P, None)]
    assert _params(alg.step) == [("rng_key", P, E), ("state", P, E), ("minibatch", P, E), ("step_size_diff", P, E),
                                 ("step_size_stoch", P, E), ("temperature", P, 1.0)]

    header = open(os.path.join(ROOT, "include", "bjx_hip.h")).read()
    assert "SGMCMC" in header
    for name in ("bjx_csgld_step", "bjx_csgld_update"):
        assert re.search(r"\bint " + name + r"\(", header) and name in _lib.SIGNATURES
    assert _lib.load().bjx_abi_version() == 7


def test_csgld_entry_points_reject_bad_arguments_without_gpu():
    from blackjax_amd import _lib

    lib = _lib.load()
    step, update = lib.bjx_csgld_step, lib.bjx_csgld_update
    step_tail = (1.0, 10.0, 0.1, None, 1.0, None) + (None,) * 5
    update_tail = (1.0, 10.0, 0.0, 0.1, None) + (None,) * 4
    assert step(None, 1, 2, 0, -1, 4, 8, 16, *step_tail) != 0
    assert b"bjx_csgld_step: null pointer" in lib.bjx_last_error()
    for n, d, m in ((-1, 8, 16), (4, 0, 16), (4, -3, 16), (4, 8, 1), (4, 8, 0), (0, 8, 1)):  # sizes before pointers
        assert step(None, 1, 2, 0, -1, n, d, m, *step_tail) != 0
        assert b"bjx_csgld_step: bad sizes" in lib.bjx_last_error()
    assert step(None, 1, 2, 0, -1, 0, 8, 2, *step_tail) == 0  # an empty batch is a no-op

    assert update(None, 4, 16, *update_tail) != 0 and b"bjx_csgld_update: null pointer" in lib.bjx_last_error()
    for n, m in ((-1, 16), (4, 1), (4, 0), (4, -2), (0, 1)):
        assert update(None, n, m, *update_tail) != 0 and b"bjx_csgld_update: bad sizes" in lib.bjx_last_error()
    assert update(None, 0, 2, *update_tail) == 0


def test_csgld_argument_errors():
    import blackjax_amd as bjx

    mod = bjx.sgmcmc.csgld
    N, D, M = 6, 4, 8
    q, key = torch.zeros(N, D), prng.key(0)  # host tensors: there is no CPU fallback
    pdf, idx = torch.full((N, M), 1.0 / M), torch.full((N,), M - 1, dtype=torch.int32)
    state = mod.ContourSGLDState(q, pdf, idx)
    alg = bjx.csgld(exact_logdensity, exact_gradient, num_partitions=M)
    with pytest.raises(RuntimeError):
        bjx.csgld.init(q)
    with pytest.raises(RuntimeError):
        alg.init(q)
    with pytest.raises(RuntimeError):
        alg.step(key, state, None, 0.1, 0.1)
    with pytest.raises(RuntimeError):
        mod.langevin_step(key, q, q, pdf, idx, 0.1)
    with pytest.raises(RuntimeError):
        mod.update_energy_histogram(torch.zeros(N), pdf, 0.1)

    # wrong-length per-chain arguments, named, wherever the tensors live
    with pytest.raises(ValueError, match="step_size_diff"):
        alg.step(key, state, None, torch.full((N + 1,), 0.1), 0.1)
    with pytest.raises(ValueError, match="step_size_stoch"):
        alg.step(key, state, None, 0.1, torch.full((N - 1,), 0.1))
    with pytest.raises(ValueError, match="temperature"):
        alg.step(key, state, None, 0.1, 0.1, torch.ones(N + 2))
    with pytest.raises(ValueError, match="step_size_diff"):
        mod.langevin_step(key, q, q, pdf, idx, torch.full((N + 1,), 0.1))
    with pytest.raises(ValueError, match="temperature"):
        mod.langevin_step(key, q, q, pdf, idx, 0.1, torch.ones(N - 1))
    with pytest.raises(ValueError, match="step_size_stoch"):
        mod.update_energy_histogram(torch.zeros(N), pdf, torch.full((N + 1,), 0.1))

    # the histogram and the index: shape and dtype
    bad_states = [(torch.zeros(N + 1, M), idx), (torch.zeros(N, M + 1), idx), (torch.zeros(N * M), idx),
                  (pdf.double(), idx), (pdf, idx.long()), (pdf, torch.zeros(N + 1, dtype=torch.int32)),
                  (pdf, torch.zeros(N, 1, dtype=torch.int32))]
    for bad_pdf, bad_idx in bad_states:
        with pytest.raises(ValueError, match="energy_pdf|energy_idx"):
            alg.step(key, mod.ContourSGLDState(q, bad_pdf, bad_idx), None, 0.1, 0.1)
    with pytest.raises(ValueError, match="energy_pdf"):
        mod.langevin_step(key, q, q, torch.zeros(N, 1), idx, 0.1)
    with pytest.raises(ValueError, match="energy_idx"):
        mod.langevin_step(key, q, q, pdf, idx.long(), 0.1)
    with pytest.raises(ValueError, match="energy_pdf"):
        mod.update_energy_histogram(torch.zeros(N), pdf[:-1], 0.1)
    with pytest.raises(ValueError):
        alg.step(key, mod.ContourSGLDState(torch.zeros(D), pdf, idx), None, 0.1, 0.1)  # not (n_chains, dim)

    for m in (1, 0):
        with pytest.raises(ValueError, match="num_partitions"):
            bjx.csgld.init(q, m)
        with pytest.raises(ValueError, match="num_partitions"):
            bjx.csgld(exact_logdensity, exact_gradient, num_partitions=m)
    for gap in (0, -1.0):
        with pytest.raises(ValueError, match="energy_gap"):
            bjx.csgld(exact_logdensity, exact_gradient, energy_gap=gap)
        with pytest.raises(ValueError, match="energy_gap"):
            bjx.csgld.build_kernel(energy_gap=gap)
        with pytest.raises(ValueError, match="energy_gap"):
            mod.langevin_step(key, q, q, pdf, idx, 0.1, energy_gap=gap)
        with pytest.raises(ValueError, match="energy_gap"):
            mod.update_energy_histogram(torch.zeros(N), pdf, 0.1, energy_gap=gap)


@pytest.mark.parametrize("M", [2, 3, 65, 512])
def test_csgld_restatement_init(M):
    """Rows are strictly decreasing, every one the same, and sum to 1 within M 2^-24 (every entry is below 1 and one
    rounding off); the index starts on the last bin."""
    st = rcs.init(np.zeros((3, 5), f32), M)
    assert st.position.dtype == st.energy_pdf.dtype == f32 and st.energy_idx.dtype == np.int32
    assert st.energy_pdf.shape == (3, M) and np.array_equal(st.energy_idx, np.full(3, M - 1))
    assert np.all(np.diff(st.energy_pdf, axis=1) < 0) and np.all(st.energy_pdf > 0)
    assert np.array_equal(st.energy_pdf[0], st.energy_pdf[2])
    assert np.all(np.abs(st.energy_pdf.astype(np.float64).sum(1) - 1.0) <= M * 2.0 ** -24)
    assert st.energy_pdf[0, 0] == f32(f32(M) / f32(M * (M + 1) // 2))


@pytest.mark.parametrize("D", [10, 260])
def test_csgld_restatement_follows_the_float64_reference_lines(D):
    """Six steps on the double well of the GPU step test (N = 33, M = 64, zeta = 0.75, chain_offset = 3): the house
    arithmetic stays within rtol = atol = 1e-6 of the reference's lines in float64.  The float64 side floors the
    log-density values of the house side, so a bin edge cannot flip an index."""
    N, M, zeta = 33, 64, 0.75
    q0, eps, eps_sa, T, mbs, gap, min_e = rcs.double_well_case(N, D)
    st, st64, history = rcs.init(q0, M), rcs.init(q0, M), []
    for k, m in zip(prng.split(prng.key(9), 6), mbs):
        seen = []

        def recorded(q, mb):
            seen.append(np.asarray(rcs.double_well_logdensity_estimator(q, mb), f32))
            return seen[-1]

        st = rcs.csgld_kernel(k, st, recorded, rcs.double_well_gradient_estimator, m, eps, eps_sa, zeta, T, gap,
                              min_e, chain_offset=3)
        st64 = rcs.csgld_kernel_f64(k, st64, lambda q, mb: seen[0], rcs.double_well_gradient_estimator, m, eps,
                                    eps_sa, zeta, T, gap, min_e, chain_offset=3)
        assert all(x.dtype == t for x, t in zip(st, (f32, f32, np.int32)))
        np.testing.assert_allclose(st.position, st64.position, rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(st.energy_pdf, st64.energy_pdf, rtol=1e-6, atol=1e-6)
        assert np.array_equal(st.energy_idx, st64.energy_idx)
        history.append(st.energy_idx)
    assert len(np.unique(np.concatenate(history))) >= 3 and not np.allclose(st.position, q0)


def test_csgld_restatement_with_zeta_zero_is_sgld():
    """zeta = 0: the multiplier is exactly 1 on a positive histogram, so the Langevin step is sgld's, bit for bit."""
    N, D, M = 33, 10, 65
    q0, eps, _, T, mbs, gap, _ = rcs.double_well_case(N, D)
    rng = np.random.default_rng(3)
    pdf = rng.uniform(0.1, 1.0, (N, M)).astype(f32)
    idx = rng.integers(1, M, N).astype(np.int32)
    g = np.asarray(rcs.double_well_gradient_estimator(q0, mbs[0]), f32)
    q1 = rcs.langevin_step(prng.key(9), q0, g, pdf, idx, eps, T, zeta=0.0, energy_gap=gap, chain_offset=3)
    expect = rsg.sgld_kernel(prng.key(9), q0, rcs.double_well_gradient_estimator, mbs[0], eps, T, chain_offset=3)
    assert q1.dtype == f32 and np.array_equal(q1.view(np.uint32), expect.view(np.uint32))
    other = rcs.langevin_step(prng.key(9), q0, g, pdf, idx, eps, T, zeta=1.0, energy_gap=gap, chain_offset=3)
    assert not np.array_equal(other, q1)


def test_csgld_restatement_histogram_is_the_running_mean_of_the_visited_bins():
    """zeta = 0 and step_size_stoch = 1 / (t + 1) at step t make the update pdf <- pdf + (e_i - pdf) / (t + 1), the
    running mean: after T = 32 steps energy_pdf is the empirical histogram of the visited indices within 4 T 2^-24
    (three roundings per step -- the step size, 1 - pdf[i], the fma -- never amplified since 1 - w <= 1, plus margin).
    The log-density estimator returns the minibatch, a prescribed energy sequence: with zeta = 0 the first update
    empties every bin but one, the next multiplier is 0 * (log 0 - log 0) = NaN as in the reference, and a
    position-dependent estimator would only ever visit bin 1 from there on."""
    N, D, M, T = 33, 10, 65, 32
    rng = np.random.default_rng(4)
    st = rcs.init(np.zeros((N, D), f32), M)
    visited = []
    for t, k in enumerate(prng.split(prng.key(11), T)):
        energies = rng.uniform(-20.0, 700.0, N).astype(f32)
        st = rcs.csgld_kernel(k, st, lambda q, mb: -mb, exact_gradient, energies, 0.01, 1.0 / (t + 1), 0, 1.0, 10, 0)
        visited.append(st.energy_idx)
    visited = np.stack(visited, 1)
    assert len(np.unique(visited)) > 30 and visited.min() == 1 and visited.max() == M - 1
    empirical = np.stack([np.bincount(v, minlength=M) for v in visited]) / T
    assert np.abs(st.energy_pdf - empirical).max() <= 4 * T * 2.0 ** -24
