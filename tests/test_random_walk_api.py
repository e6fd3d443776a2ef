"""``blackjax_amd.rmh`` / ``additive_step_random_walk`` / ``irmh``: API surface, C-ABI argument checks (no GPU needed)
and the NumPy restatement the GPU tests hold the kernels against (tests/random_walk_restatement.py), pinned on its own
as a sampler and for the orientation of ``proposal_logdensity_fn``."""
import numpy as np
import pytest

import random_walk_restatement as rrw
from oracle import prng, targets as otargets

f32 = np.float32
SIG = np.array([0.5, 1.0, 2.0, 4.0], f32)
N_ENSEMBLE = 4096


def _target():
    return otargets.diag_gaussian((f32(1) / (SIG * SIG)).astype(f32))


def _start():
    return (prng.normal(prng.key(11), (N_ENSEMBLE, SIG.size)) * SIG).astype(f32)


def _moment_errors(x):
    """|mean| and |var / sigma^2 - 1| of the ensemble in standard errors of N independent draws of the target (the
    bounds of test_mala_restatement_is_a_correct_sampler: both must be <= 5)."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    mean_se = np.abs(x.mean(0)) / (SIG / np.sqrt(n))
    var_se = np.abs(x.var(0, ddof=1) / (SIG.astype(np.float64) ** 2) - 1.0) / np.sqrt(2.0 / (n - 1))
    return mean_se, var_se


def test_random_walk_api_surface():
    import importlib

    import blackjax_amd as bjx

    prw = importlib.import_module("blackjax_amd.random_walk")
    pirmh = importlib.import_module("blackjax_amd.irmh")  # (the package attribute ``irmh`` is the API object)
    for name in ("rmh", "irmh", "additive_step_random_walk", "normal_random_walk"):
        assert name in bjx.__all__ and callable(getattr(bjx, name))
    for api in (bjx.rmh, bjx.irmh, bjx.additive_step_random_walk):
        assert isinstance(api, bjx.GenerateSamplingAPI) and callable(api.init) and callable(api.build_kernel)
    assert bjx.rmh.init is prw.init and bjx.rmh.build_kernel is prw.build_rmh
    assert bjx.additive_step_random_walk.init is prw.init
    assert bjx.additive_step_random_walk.build_kernel is prw.build_additive_step
    assert bjx.additive_step_random_walk.normal_random_walk is prw.normal_random_walk
    assert bjx.normal_random_walk is prw.normal_random_walk
    assert bjx.irmh.init is pirmh.init and pirmh.init is prw.init and bjx.irmh.build_kernel is pirmh.build_kernel
    assert prw.RWState._fields == ("position", "logdensity")
    assert prw.RWInfo._fields == ("acceptance_rate", "is_accepted", "proposal")
    assert rrw.RWState._fields == prw.RWState._fields and rrw.RWInfo._fields == prw.RWInfo._fields
    assert pirmh.RWState is prw.RWState and pirmh.RWInfo is prw.RWInfo
    assert callable(bjx.random.chain_normal) and "chain_normal" in bjx.random.__all__

    def logp(q):
        return -0.5 * (q * q).sum(-1)

    algs = [bjx.normal_random_walk(logp, 0.5), bjx.additive_step_random_walk(logp, prw.normal(0.5)),
            bjx.additive_step_random_walk.normal_random_walk(logp, 0.5, chain_offset=2),
            bjx.rmh(logp, lambda k, q: q), bjx.rmh(logp, lambda k, q: q, lambda a, b: a.logdensity, chain_offset=1),
            bjx.irmh(logp, lambda k: None), bjx.irmh(logp, lambda k: None, lambda a, b: a.logdensity, chain_offset=1)]
    for alg in algs:
        assert isinstance(alg, bjx.SamplingAlgorithm) and callable(alg.init) and callable(alg.step)
    for build in (bjx.rmh.build_kernel, bjx.irmh.build_kernel, bjx.additive_step_random_walk.build_kernel):
        assert callable(build())


def test_random_walk_entry_points_reject_bad_arguments_without_gpu():
    from blackjax_amd import _lib

    lib = _lib.load()
    for name in ("bjx_rw_noise", "bjx_rw_propose", "bjx_rw_finish", "bjx_smc_temper_value"):
        assert name in _lib.SIGNATURES
    one = 16  # a non-null (never dereferenced: every call below is rejected before any launch) 16-byte aligned address
    rc = lib.bjx_rw_noise(None, 1, 2, 0, -1, -1, 4, 8, None)
    assert rc != 0 and b"bjx_rw_noise: null pointer" in lib.bjx_last_error()
    rc = lib.bjx_rw_propose(None, 1, 2, 0, -1, 4, 8, 0.1, None, None, None, None)
    assert rc != 0 and b"bjx_rw_propose: null pointer" in lib.bjx_last_error()
    rc = lib.bjx_rw_finish(None, 1, 2, 0, -1, 4, 8, *([None] * 10))
    assert rc != 0 and b"bjx_rw_finish: null pointer" in lib.bjx_last_error()
    rc = lib.bjx_smc_temper_value(None, 4, None, None, None, None)
    assert rc != 0 and b"bjx_smc_temper_value: null pointer" in lib.bjx_last_error()
    for n, d in ((-1, 8), (4, 0), (4, -3)):  # sizes are checked before the pointers
        rc = lib.bjx_rw_noise(None, 1, 2, 0, -1, -1, n, d, None)
        assert rc != 0 and b"bjx_rw_noise: bad sizes" in lib.bjx_last_error()
        rc = lib.bjx_rw_propose(None, 1, 2, 0, -1, n, d, 0.1, None, None, None, None)
        assert rc != 0 and b"bjx_rw_propose: bad sizes" in lib.bjx_last_error()
        rc = lib.bjx_rw_finish(None, 1, 2, 0, -1, n, d, *([None] * 10))
        assert rc != 0 and b"bjx_rw_finish: bad sizes" in lib.bjx_last_error()
    rc = lib.bjx_smc_temper_value(None, -1, None, None, None, None)
    assert rc != 0 and b"bjx_smc_temper_value: bad sizes" in lib.bjx_last_error()
    for child in (-2, 2):  # the chain key itself (-1) or one of the two children of its split
        rc = lib.bjx_rw_noise(None, 1, 2, 0, -1, child, 4, 8, None)
        assert rc != 0 and b"bjx_rw_noise: bad sizes" in lib.bjx_last_error()
    # exactly one of the two proposal log-densities: an argument error, in either position
    for f_ip, f_pi in ((one, None), (None, one)):
        rc = lib.bjx_rw_finish(None, 1, 2, 0, -1, 4, 8, one, one, one, one, f_ip, f_pi, 2 * one, 2 * one, one, one)
        assert rc != 0 and b"bjx_rw_finish: f_init_prop and f_prop_init go together" in lib.bjx_last_error()
    # a diagonal scale and a ready-made move exclude each other
    rc = lib.bjx_rw_propose(None, 1, 2, 0, -1, 4, 8, 0.1, one, one, one, 2 * one)
    assert rc != 0 and b"bjx_rw_propose: sigma_diag and move_lin are exclusive" in lib.bjx_last_error()
    # an empty batch is accepted before any pointer is looked at
    assert lib.bjx_rw_noise(None, 1, 2, 0, -1, -1, 0, 8, None) == 0
    assert lib.bjx_rw_propose(None, 1, 2, 0, -1, 0, 8, 0.1, None, None, None, None) == 0
    assert lib.bjx_rw_finish(None, 1, 2, 0, -1, 0, 8, *([None] * 10)) == 0
    assert lib.bjx_smc_temper_value(None, 0, None, None, None, None) == 0


def test_normal_validates_sigma():
    import torch

    from blackjax_amd import random_walk as prw

    with pytest.raises(ValueError):
        prw.normal(torch.ones(2, 3, 3))  # ndim 3
    with pytest.raises(ValueError):
        prw.normal(np.ones((5, 3), f32))  # a 2-d sigma is a matrix: it must be square
    for ok in (0.5, np.float32(0.5), torch.tensor(0.5), np.ones(3, f32), torch.eye(3)):
        assert callable(prw.normal(ok))
    with pytest.raises(ValueError):
        rrw.normal(np.ones((5, 3), f32))
    with pytest.raises(ValueError):
        rrw.normal(np.ones((2, 3, 3), f32))


def _run_normal_random_walk(always_accept, n_steps=50):
    fn = _target()
    st = rrw.init(_start(), fn)
    step = rrw.normal((f32(0.8) * SIG).astype(f32))
    rates = []
    for k in prng.split(prng.key(12), n_steps):
        st, info = rrw.additive_step_kernel(k, st, fn, step, always_accept=always_accept)
        assert info.acceptance_rate.dtype == f32 and info.is_accepted.dtype == bool
        assert info.proposal.position.shape == st.position.shape
        rates.append(info.acceptance_rate.mean())
    return st, float(np.mean(rates))


def test_random_walk_restatement_is_a_correct_sampler():
    """4 096 independent chains started IN the target (a diagonal Gaussian, sigma = 0.5, 1, 2, 4) stay in it under a
    correct random-walk Metropolis kernel with steps 0.8 sigma, so after 50 transitions the ensemble mean and variance
    of every dimension are those of 4 096 independent draws: |mean| <= 5 sigma / sqrt(N),
    |var / sigma^2 - 1| <= 5 sqrt(2 / (N - 1)).  A chain that accepts every proposal is a plain random walk: its
    variance grows by 0.64 sigma^2 per transition, to 33 sigma^2 -- over a thousand standard errors."""
    fn = _target()
    st, rate = _run_normal_random_walk(False)
    mean_se, var_se = _moment_errors(st.position)
    print("mean (s.e.):", mean_se, "var (s.e.):", var_se, "acceptance:", rate)
    assert np.all(mean_se <= 5.0), mean_se
    assert np.all(var_se <= 5.0), var_se
    assert 0.1 < rate < 0.9  # both branches of the accept are taken
    assert np.array_equal(fn(st.position)[0], st.logdensity)  # the state is consistent

    broken, _ = _run_normal_random_walk(True)
    _, var_broken = _moment_errors(broken.position)
    print("accepting every proposal, var (s.e.):", var_broken)
    assert np.all(var_broken > 5.0), var_broken


def _irmh_run(swap, n_steps=5):
    fn = _target()

    def draw(rng_key, keys):
        return (SIG * rrw.chain_normal(keys, SIG.size, child=0)).astype(f32)

    def logq(a, b):  # the log-density of proposing b from a: the proposal ignores a
        return fn(b.position)[0]

    f = (lambda a, b: logq(b, a)) if swap else logq
    st = rrw.init(_start()[:512], fn)
    rates = []
    for k in prng.split(prng.key(13), n_steps):
        st, info = rrw.irmh_kernel(k, st, fn, draw, f)
        rates.append(info.acceptance_rate)
    return np.stack(rates)


def test_proposal_logdensity_orientation_irmh():
    """``proposal_logdensity_fn(a, b)`` is the log-density of proposing ``b`` FROM ``a``.  An independent proposal that
    IS the target, with ``f(a, b) = log q(b.position)``, is accepted with probability 1 on every chain and transition
    (the two energies are the same two numbers summed in the other order); with the arguments swapped the ratio is
    ``(p(q1) / p(q0))^2`` and is not."""
    rates = _irmh_run(False)
    assert rates.shape == (5, 512) and np.all(rates >= 1.0 - 1e-5), rates.min()
    swapped = _irmh_run(True)
    print("swapped arguments: acceptance rate min", swapped.min(), "mean", swapped.mean())
    assert not np.all(swapped >= 1.0 - 1e-5)
    assert swapped.mean() < 0.9


DRIFT, DRIFT_SCALE = f32(0.5), f32(0.7)


def _drift_run(with_f, n_steps=50):
    fn = _target()

    def generator(rng_key, keys, position):  # q1 = q0 + 0.5 + 0.7 z
        z = rrw.chain_normal(keys, position.shape[1], child=0)
        return ((position + DRIFT).astype(f32) + (DRIFT_SCALE * z).astype(f32)).astype(f32)

    def f(a, b):  # log N(b | a + 0.5, 0.7^2 I) up to its constant
        r = (b.position.astype(np.float64) - a.position.astype(np.float64) - float(DRIFT)) / float(DRIFT_SCALE)
        return (-0.5 * np.sum(r * r, axis=-1)).astype(f32)

    st = rrw.init(_start(), fn)
    rates = []
    for k in prng.split(prng.key(14), n_steps):
        st, info = rrw.rmh_kernel(k, st, fn, generator, f if with_f else None)
        rates.append(info.acceptance_rate.mean())
    return st, float(np.mean(rates))


def test_proposal_logdensity_orientation_drifting_rmh():
    """A proposal that drifts, ``q1 = q0 + 0.5 + 0.7 z``, corrected by the matching ``f``, leaves the target invariant:
    the ensemble mean stays within 5 standard errors (the variance too).  Without ``f`` -- or with it the wrong way
    round, which doubles the error instead of cancelling it -- every chain is pushed upwards and the mean leaves the
    bound."""
    st, rate = _drift_run(True)
    mean_se, var_se = _moment_errors(st.position)
    print("with f: mean (s.e.):", mean_se, "var (s.e.):", var_se, "acceptance:", rate)
    assert np.all(mean_se <= 5.0), mean_se
    assert np.all(var_se <= 5.0), var_se
    assert 0.05 < rate < 0.95
    bad, _ = _drift_run(False)
    mean_bad, _ = _moment_errors(bad.position)
    print("without f: mean (s.e.):", mean_bad)
    assert np.any(mean_bad > 5.0), mean_bad
