"""``blackjax_amd.elliptical_slice``: API surface, argument checks and C-ABI argument checks (no GPU needed), and the
NumPy restatement the GPU tests hold the kernels against (tests/elliptical_slice_restatement.py), pinned on its own
as a sampler."""
import numpy as np
import pytest
import torch

import elliptical_slice_restatement as ress
from elliptical_slice_restatement import COV, MEAN, conjugate_loglik, moment_errors, posterior_draws
from oracle import prng

f32 = np.float32


def test_elliptical_slice_api_surface():
    import importlib

    import blackjax_amd as bjx

    pess = importlib.import_module("blackjax_amd.elliptical_slice")  # (the package attribute is the API object)
    assert "elliptical_slice" in bjx.__all__
    ess = bjx.elliptical_slice
    assert callable(ess) and callable(ess.init) and callable(ess.build_kernel)
    assert ess.init is pess.init and ess.build_kernel is pess.build_kernel
    assert pess.EllipSliceState._fields == ("position", "logdensity")
    assert pess.EllipSliceInfo._fields == ("momentum", "theta", "subiter")
    assert ress.EllipSliceState._fields == pess.EllipSliceState._fields
    assert ress.EllipSliceInfo._fields == pess.EllipSliceInfo._fields
    alg = ess(lambda q: -0.5 * (q * q).sum(-1), mean=0.0, cov=torch.ones(4))
    assert isinstance(alg, bjx.SamplingAlgorithm) and callable(alg.init) and callable(alg.step)
    assert callable(ess.build_kernel(torch.eye(4), torch.zeros(4)))


def test_elliptical_slice_argument_checks_without_gpu():
    """Shape errors of ``mean`` / ``cov`` are raised from host-side shapes, before any device is touched; a host
    tensor with a well-formed prior then meets ``check_batch``'s error (there is no CPU fallback)."""
    import blackjax_amd as bjx
    from blackjax_amd.elliptical_slice import EllipSliceState

    ess = bjx.elliptical_slice
    N, D = 3, 4
    fn = lambda q: -0.5 * (q * q).sum(-1)
    st = EllipSliceState(torch.zeros(N, D), torch.zeros(N))  # host tensors: shapes only
    key = prng.key(1)

    def step(mean, cov):
        return ess(fn, mean=mean, cov=cov).step(key, st)

    with pytest.raises(ValueError, match="cov has 5 entries, position has 4"):
        step(0.0, torch.ones(D + 1))
    with pytest.raises(ValueError, match="position has 4 dims"):
        step(0.0, torch.eye(D + 1))
    with pytest.raises(ValueError, match="must be square"):
        step(0.0, torch.ones(N, D))  # a 2-d cov is always dense: never read as per-chain diagonals
    with pytest.raises(ValueError, match="wrong number of dimensions"):
        step(0.0, torch.ones(()))
    with pytest.raises(ValueError, match="wrong number of dimensions"):
        step(0.0, torch.ones(2, 2, 2, 2))
    with pytest.raises(ValueError, match="mean has 3 entries, position has 4"):
        step(torch.zeros(D - 1), torch.ones(D))
    with pytest.raises(NotImplementedError, match="per-chain mean"):
        step(torch.zeros(N, D), torch.ones(D))
    with pytest.raises(NotImplementedError, match="per-chain cov"):
        step(0.0, torch.ones(N, D, D))
    with pytest.raises(ValueError):
        ess(fn, mean=0.0, cov=torch.ones(D)).step(key, EllipSliceState(torch.zeros(D), torch.zeros(())))
    for mean, cov in ((0.0, torch.ones(D)), (torch.zeros(D), torch.eye(D)), (np.zeros(D, f32), np.ones(D, f32))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            step(mean, cov)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ess(fn, mean=0.0, cov=torch.ones(D)).init(torch.zeros(N, D))


def test_elliptical_slice_entry_points_reject_bad_arguments_without_gpu():
    from blackjax_amd import _lib

    lib = _lib.load()
    names = ("bjx_ess_begin", "bjx_ess_noise", "bjx_ess_shrink")
    n_ptr = {"bjx_ess_begin": 13, "bjx_ess_noise": 1, "bjx_ess_shrink": 16}
    for name in names:
        assert name in _lib.SIGNATURES
        fn = getattr(lib, name)
        rc = fn(None, 1, 2, 0, -1, 4, 8, *([None] * n_ptr[name]))
        assert rc != 0 and (name + ": null pointer").encode() in lib.bjx_last_error()
        for n, d in ((-1, 8), (4, 0), (4, -3)):  # sizes are checked before the pointers
            rc = fn(None, 1, 2, 0, -1, n, d, *([None] * n_ptr[name]))
            assert rc != 0 and (name + ": bad sizes").encode() in lib.bjx_last_error()
        assert fn(None, 1, 2, 0, -1, 0, 8, *([None] * n_ptr[name])) == 0  # an empty batch is a no-op
    # begin takes the diagonal of cov or the ready dense product, never both and never neither (any non-null
    # addresses do: the check comes before the launch)
    p = 16
    rc = lib.bjx_ess_begin(None, 1, 2, 0, -1, 4, 8, p, p, p, *([p] * 10))
    assert rc != 0 and b"exactly one of cov_diag and nu_lin" in lib.bjx_last_error()
    rc = lib.bjx_ess_begin(None, 1, 2, 0, -1, 4, 8, p, None, None, *([p] * 10))
    assert rc != 0 and b"exactly one of cov_diag and nu_lin" in lib.bjx_last_error()


def test_elliptical_slice_restatement_is_a_correct_sampler():
    """4 096 independent chains started IN the posterior of the conjugate case stay in it under a correct kernel, so
    after 30 transitions the ensemble mean and variance of every coordinate are those of 4 096 independent draws:
    within 5 standard errors, sqrt(var / N) for the mean and var sqrt(2 / (N - 1)) for the variance.  A prior mean
    entered in the wrong place (the ellipse not centred on it) moves the means by tens of standard errors."""
    N, T = 4096, 30
    mean, cov = MEAN.astype(f32), COV.astype(f32)
    st = ress.init(posterior_draws(N), conjugate_loglik)
    counts = []
    for k in prng.split(prng.key(7), T):
        st, info = ress.kernel(k, st, conjugate_loglik, mean=mean, cov=cov)
        assert info.subiter.dtype == np.int32 and info.theta.dtype == f32 and info.momentum.dtype == f32
        assert np.all(info.subiter >= 1)
        counts.append(info.subiter)
    counts = np.concatenate(counts)
    mean_se, var_se = moment_errors(st.position)
    print("mean (s.e.):", mean_se, "var (s.e.):", var_se, "subiter mean / max:", counts.mean(), counts.max())
    assert np.all(mean_se <= 5.0), mean_se
    assert np.all(var_se <= 5.0), var_se
    assert np.any(counts == 1) and np.any(counts >= 3)  # first-proposal accepts and repeated shrinking both occur
    assert np.array_equal(conjugate_loglik(st.position), st.logdensity)  # the state is consistent
