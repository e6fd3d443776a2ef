"""``blackjax_amd.barker``: API surface, C-ABI argument checks (no GPU needed) and the NumPy restatement the GPU
tests hold the kernels against (tests/barker_restatement.py), pinned on its own as a sampler."""
import inspect
import os
import re

import numpy as np

import barker_restatement as rbarker
from oracle import prng, targets as otargets

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_barker_api_surface():
    import importlib

    import blackjax_amd as bjx

    pbarker = importlib.import_module("blackjax_amd.barker")  # (the package attribute ``barker`` is the API object)
    assert "barker" in bjx.__all__ and "barker_proposal" in bjx.__all__
    assert bjx.barker_proposal is bjx.barker
    assert callable(bjx.barker) and callable(bjx.barker.init) and callable(bjx.barker.build_kernel)
    assert bjx.barker.init is pbarker.init and bjx.barker.build_kernel is pbarker.build_kernel
    assert pbarker.BarkerState._fields == ("position", "logdensity", "logdensity_grad")
    assert pbarker.BarkerInfo._fields == ("acceptance_rate", "is_accepted", "proposal")
    assert rbarker.BarkerState._fields == pbarker.BarkerState._fields
    assert rbarker.BarkerInfo._fields == pbarker.BarkerInfo._fields
    alg = bjx.barker(lambda q: -0.5 * (q * q).sum(-1), 0.1)
    assert isinstance(alg, bjx.SamplingAlgorithm) and callable(alg.init) and callable(alg.step)
    assert list(inspect.signature(alg.init).parameters)[:1] == ["position"]
    assert list(inspect.signature(alg.step).parameters) == ["rng_key", "state"]
    kernel = bjx.barker.build_kernel()
    assert list(inspect.signature(kernel).parameters) == ["rng_key", "state", "logdensity_fn", "step_size",
                                                          "inverse_mass_matrix", "chain_offset"]
    assert list(inspect.signature(pbarker.as_top_level_api).parameters) == ["logdensity_fn", "step_size",
                                                                            "inverse_mass_matrix", "chain_offset"]


def test_barker_entry_points_declared_and_reject_bad_arguments_without_gpu():
    from blackjax_amd import _lib

    header = open(os.path.join(ROOT, "include", "bjx_hip.h")).read()
    for name in ("bjx_barker_propose", "bjx_barker_finish"):
        assert re.search(r"\bint " + name + r"\(", header) and name in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.bjx_abi_version() == 7  # additive
    rc = lib.bjx_barker_propose(None, 1, 2, 0, -1, 4, 8, 0.1, None, None, 0, None, None, None)
    assert rc != 0 and b"bjx_barker_propose: null pointer" in lib.bjx_last_error()
    rc = lib.bjx_barker_finish(None, 1, 2, 0, -1, 4, 8, *([None] * 11))
    assert rc != 0 and b"bjx_barker_finish: null pointer" in lib.bjx_last_error()
    for n, d in ((-1, 8), (4, 0), (4, -3)):  # sizes are checked before the pointers
        rc = lib.bjx_barker_propose(None, 1, 2, 0, -1, n, d, 0.1, None, None, 0, None, None, None)
        assert rc != 0 and b"bjx_barker_propose: bad sizes" in lib.bjx_last_error()
        rc = lib.bjx_barker_finish(None, 1, 2, 0, -1, n, d, *([None] * 11))
        assert rc != 0 and b"bjx_barker_finish: bad sizes" in lib.bjx_last_error()
    # an empty batch is a no-op that touches no pointer
    assert lib.bjx_barker_propose(None, 1, 2, 0, -1, 0, 8, 0.1, None, None, 0, None, None, None) == 0
    assert lib.bjx_barker_finish(None, 1, 2, 0, -1, 0, 8, *([None] * 11)) == 0


def test_barker_restatement_is_a_correct_sampler():
    """4 096 independent chains started IN the target (a diagonal Gaussian in D = 8, variances 0.25 * 16^(j / 7):
    0.25 ... 4, handed to the kernel as its inverse mass matrix) stay in it under a correct Barker kernel, so after
    200 transitions the ensemble mean and variance of every dimension are those of 4 096 independent draws:
    |mean| <= 5 sigma / sqrt(N), |var / sigma^2 - 1| <= 5 sqrt(2 / (N - 1)).  Step size 1.0: mean acceptance 0.62."""
    D, N, tau = 8, 4096, 1.0
    var = (0.25 * 16.0 ** (np.arange(D) / (D - 1))).astype(f32)
    sig = np.sqrt(var).astype(f32)
    fn = otargets.diag_gaussian((f32(1) / var).astype(f32))
    q0 = (prng.normal(prng.key(11), (N, D)) * sig).astype(f32)
    st = rbarker.init(q0, fn)
    rates = []
    for k in prng.split(prng.key(12), 200):
        st, info = rbarker.kernel(k, st, fn, tau, var)
        assert info.acceptance_rate.dtype == f32 and info.is_accepted.dtype == bool
        rates.append(info.acceptance_rate.mean())
    x = st.position.astype(np.float64)
    mean_se = np.abs(x.mean(0)) / (sig / np.sqrt(N))
    var_se = np.abs(x.var(0, ddof=1) / var.astype(np.float64) - 1.0) / np.sqrt(2.0 / (N - 1))
    print("mean (s.e.):", mean_se, "var (s.e.):", var_se, "acceptance:", float(np.mean(rates)))
    assert np.all(mean_se <= 5.0), mean_se
    assert np.all(var_se <= 5.0), var_se
    assert 0.3 < float(np.mean(rates)) < 0.7  # both branches of the accept are taken
    lp, g = fn(st.position)
    assert np.array_equal(lp, st.logdensity) and np.array_equal(g, st.logdensity_grad)  # the state is consistent
    assert np.array_equal(fn(info.proposal.position)[0], info.proposal.logdensity)


def test_barker_restatement_moves_uphill():
    """The signs follow the gradient: on a unit Gaussian shifted to mu = 1.5 with chains drawn around 0, the
    increments z b - z (1 - b) sum to a positive inner product with the gradient, and the fraction of elements moved
    uphill exceeds 1/2 by many standard errors (an element moves uphill with probability expit(|z g|) >= 1/2; a
    sign-blind proposal gives 1/2 +- 1 / (2 sqrt(N D)))."""
    N, D, tau = 512, 16, 0.8
    q0 = prng.normal(prng.key(3), (N, D)).astype(f32)
    g0 = (f32(1.5) - q0).astype(f32)  # gradient of -1/2 |q - mu|^2
    q1, b, z = rbarker.propose(prng.split(prng.key(4), N), q0, g0, tau)
    step = (q1 - q0).astype(np.float64)
    np.testing.assert_array_equal(q1, np.where(b, (q0 + z).astype(f32), (q0 - z).astype(f32)))
    moved = (z != 0) & (g0 != 0)
    uphill = (step * g0 > 0)[moved]
    frac, se = uphill.mean(), 0.5 / np.sqrt(uphill.size)
    print("uphill fraction:", frac, "s.e.:", se, "sum step * g:", float((step * g0).sum()))
    assert float((step * g0).sum()) > 0
    assert frac > 0.5 + 10 * se
    # and the per-element outcomes are both taken
    assert 0 < int(b.sum()) < b.size

