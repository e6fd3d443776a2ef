"""``blackjax_amd.mala``: API surface, C-ABI argument checks (no GPU needed) and the NumPy restatement the GPU
tests hold the kernels against (tests/mala_restatement.py), pinned on its own as a sampler."""
import numpy as np

import mala_restatement as rmala
from oracle import prng, targets as otargets

f32 = np.float32


def test_mala_api_surface():
    import importlib

    import blackjax_amd as bjx

    pmala = importlib.import_module("blackjax_amd.mala")  # (the package attribute ``mala`` is the API object)
    assert "mala" in bjx.__all__
    assert callable(bjx.mala) and callable(bjx.mala.init) and callable(bjx.mala.build_kernel)
    assert bjx.mala.init is pmala.init and bjx.mala.build_kernel is pmala.build_kernel
    assert pmala.MALAState._fields == ("position", "logdensity", "logdensity_grad")
    assert pmala.MALAInfo._fields == ("acceptance_rate", "is_accepted")
    assert rmala.MALAState._fields == pmala.MALAState._fields and rmala.MALAInfo._fields == pmala.MALAInfo._fields
    alg = bjx.mala(lambda q: -0.5 * (q * q).sum(-1), 0.1)
    assert isinstance(alg, bjx.SamplingAlgorithm) and callable(alg.init) and callable(alg.step)
    assert callable(bjx.mala.build_kernel())


def test_mala_entry_points_reject_bad_arguments_without_gpu():
    from blackjax_amd import _lib

    lib = _lib.load()
    assert "bjx_mala_propose" in _lib.SIGNATURES and "bjx_mala_finish" in _lib.SIGNATURES
    rc = lib.bjx_mala_propose(None, 1, 2, 0, -1, 4, 8, 0.1, None, None, None, None)
    assert rc != 0 and b"bjx_mala_propose" in lib.bjx_last_error()
    rc = lib.bjx_mala_finish(None, 1, 2, 0, -1, 4, 8, 0.1, None, *([None] * 11))
    assert rc != 0 and b"bjx_mala_finish" in lib.bjx_last_error()
    for n, d in ((-1, 8), (4, 0), (4, -3)):  # sizes are checked before the pointers
        rc = lib.bjx_mala_propose(None, 1, 2, 0, -1, n, d, 0.1, None, None, None, None)
        assert rc != 0 and b"bjx_mala_propose: bad sizes" in lib.bjx_last_error()
        rc = lib.bjx_mala_finish(None, 1, 2, 0, -1, n, d, 0.1, None, *([None] * 11))
        assert rc != 0 and b"bjx_mala_finish: bad sizes" in lib.bjx_last_error()


def test_mala_restatement_is_a_correct_sampler():
    """4 096 independent chains started IN the target (a diagonal Gaussian, sigma = 0.5, 1, 2, 4) stay in it under a
    correct MALA kernel, so after 50 transitions the ensemble mean and variance of every dimension are those of
    4 096 independent draws: |mean| <= 5 sigma / sqrt(N), |var / sigma^2 - 1| <= 5 sqrt(2 / (N - 1)).  A chain that
    accepts every proposal (unadjusted Langevin) inflates the variance of the stiffest dimension by
    1 / (1 - tau / (2 sigma^2)) = 1.43 at tau = 0.15: ~20 standard errors."""
    sig = np.array([0.5, 1.0, 2.0, 4.0], f32)
    N, tau = 4096, 0.15
    fn = otargets.diag_gaussian((f32(1) / (sig * sig)).astype(f32))
    q0 = (prng.normal(prng.key(11), (N, sig.size)) * sig).astype(f32)
    st = rmala.init(q0, fn)
    rates = []
    for k in prng.split(prng.key(12), 50):
        st, info = rmala.kernel(k, st, fn, tau)
        assert info.acceptance_rate.dtype == f32 and info.is_accepted.dtype == bool
        rates.append(info.acceptance_rate.mean())
    x = st.position.astype(np.float64)
    mean_se = np.abs(x.mean(0)) / (sig / np.sqrt(N))
    var_se = np.abs(x.var(0, ddof=1) / (sig.astype(np.float64) ** 2) - 1.0) / np.sqrt(2.0 / (N - 1))
    print("mean (s.e.):", mean_se, "var (s.e.):", var_se, "acceptance:", float(np.mean(rates)))
    assert np.all(mean_se <= 5.0), mean_se
    assert np.all(var_se <= 5.0), var_se
    assert 0.5 < float(np.mean(rates)) < 1.0  # both branches of the accept are taken
    lp, g = fn(st.position)
    assert np.array_equal(lp, st.logdensity) and np.array_equal(g, st.logdensity_grad)  # the state is consistent
