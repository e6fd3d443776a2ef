"""``blackjax_amd.orbital_hmc``: API surface, C-ABI argument checks (no GPU needed) and the NumPy restatement the GPU
tests hold the kernels against (tests/orbital_hmc_restatement.py): its invariants, and the sampler it states pinned on
its own on a periodic flow."""
import inspect
import os

import numpy as np

import orbital_hmc_restatement as ro
from oracle import prng, targets as otargets

f32 = np.float32


def test_orbital_hmc_api_surface():
    import blackjax_amd as bjx
    from blackjax_amd import integrators, periodic_orbital as po

    assert "orbital_hmc" in bjx.__all__ and "periodic_orbital" in bjx.__all__
    assert inspect.ismodule(bjx.periodic_orbital) and bjx.periodic_orbital is po
    assert callable(bjx.orbital_hmc) and bjx.orbital_hmc.init is po.init and bjx.orbital_hmc.build_kernel is po.build_kernel
    assert po.PeriodicOrbitalState._fields == ("positions", "weights", "directions", "logdensities", "logdensities_grad")
    assert po.PeriodicOrbitalInfo._fields == ("momentums", "weights_mean", "weights_variance")
    assert ro.PeriodicOrbitalState._fields == po.PeriodicOrbitalState._fields
    assert ro.PeriodicOrbitalInfo._fields == po.PeriodicOrbitalInfo._fields
    for name in po.__all__:
        assert hasattr(po, name)

    assert list(inspect.signature(po.init).parameters) == ["position", "logdensity_fn", "period"]
    sig = inspect.signature(po.build_kernel)
    assert list(sig.parameters) == ["bijection"] and sig.parameters["bijection"].default is integrators.velocity_verlet
    sig = inspect.signature(po.build_kernel())
    assert list(sig.parameters) == ["rng_key", "state", "logdensity_fn", "step_size", "inverse_mass_matrix", "period",
                                    "chain_offset"]
    assert sig.parameters["chain_offset"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["chain_offset"].default == 0
    sig = inspect.signature(po.as_top_level_api)
    assert list(sig.parameters) == ["logdensity_fn", "step_size", "inverse_mass_matrix", "period", "bijection",
                                    "chain_offset"]
    for name in ("bijection", "chain_offset"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["bijection"].default is integrators.velocity_verlet and sig.parameters["chain_offset"].default == 0

    alg = bjx.orbital_hmc(lambda q: -0.5 * (q * q).sum(-1), 0.1, np.ones(3, f32), 4)
    assert isinstance(alg, bjx.SamplingAlgorithm) and callable(alg.init) and callable(alg.step)
    assert list(inspect.signature(alg.init).parameters) == ["position", "rng_key"]
    assert inspect.signature(alg.init).parameters["rng_key"].default is None


def test_orbital_entry_points_reject_bad_arguments_without_gpu():
    from blackjax_amd import _lib

    lib = _lib.load()
    assert "bjx_orbital_open" in _lib.SIGNATURES and "bjx_orbital_finish" in _lib.SIGNATURES
    assert hasattr(lib, "bjx_orbital_open") and hasattr(lib, "bjx_orbital_finish")
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "bjx_hip.h")).read()
    assert "int bjx_orbital_open(" in header and "int bjx_orbital_finish(" in header and "Periodic orbital" in header

    def open_(n, p, d, stride=0):
        return lib.bjx_orbital_open(None, 1, 2, 0, -1, n, p, d, 1, 0.1, None, None, stride, *([None] * 11))

    def finish(n, p, d, stride=0):
        return lib.bjx_orbital_finish(None, n, p, d, 1, None, stride, *([None] * 9))

    assert open_(4, 3, 8) != 0 and b"bjx_orbital_open" in lib.bjx_last_error()
    assert finish(4, 3, 8) != 0 and b"bjx_orbital_finish" in lib.bjx_last_error()
    for n, p, d, stride in ((-1, 3, 8, 0), (4, 0, 8, 0), (4, 3, 0, 0), (4, -2, 8, 0), (4, 3, 8, 5)):  # sizes come first
        assert open_(n, p, d, stride) != 0 and b"bjx_orbital_open: bad sizes" in lib.bjx_last_error()
        assert finish(n, p, d, stride) != 0 and b"bjx_orbital_finish: bad sizes" in lib.bjx_last_error()
    assert open_(0, 3, 8) == 0 and finish(0, 3, 8) == 0  # an empty batch is a no-op


def _small_case(N=64, D=5, seed=3):
    sig = (10.0 ** (-0.5 + np.arange(D) / max(D - 1, 1))).astype(f32)
    inv_var = (f32(1) / (sig * sig)).astype(f32)
    q0 = (prng.normal(prng.key(seed), (N, D)) * sig).astype(f32)
    imm = np.linspace(0.5, 2.0, D).astype(f32)
    return inv_var, q0, imm


def test_orbital_restatement_invariants():
    """P = 1 returns the incoming state with weight 1 and variance 0; for P > 1 slot d of the new orbit IS the selected
    state (signed step 0) bit for bit; weights sum to 1; rows on which the target returns NaN get weight exactly 0 and
    no NaN reaches any weight."""
    inv_var, q0, imm = _small_case()
    fn = otargets.diag_gaussian(inv_var)
    N, D = q0.shape

    st0 = ro.init(q0, fn, 1)
    st, info, ch = ro.kernel(prng.key(5), st0, fn, f32(0.2), imm, 1)
    for a, b in zip(st, st0):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert np.array_equal(st.weights, np.ones((N, 1), f32)) and np.array_equal(info.weights_variance, np.zeros(N, f32))
    assert np.array_equal(info.weights_mean, np.ones(N, f32)) and np.array_equal(ch, np.zeros(N, np.int64))

    P = 6
    eps = (f32(0.05) * np.random.default_rng(0).uniform(0.6, 1.6, N)).astype(f32)
    st = ro.init(q0, fn, P)
    assert np.array_equal(st.weights, np.full((N, P), f32(1) / f32(P))) and st.directions.dtype == np.int32
    rows = np.arange(N)
    seen = set()
    for k in prng.split(prng.key(6), 4):
        new, info, ch = ro.kernel(k, st, fn, eps, imm, P, chain_offset=2)
        d = st.directions[rows, ch]
        assert np.array_equal(d, ch)  # directions are arange(P)
        assert np.array_equal(new.positions[rows, d], st.positions[rows, ch])
        assert np.array_equal(new.logdensities[rows, d], st.logdensities[rows, ch])
        assert np.array_equal(new.logdensities_grad[rows, d], st.logdensities_grad[rows, ch])
        p_sel = info.momentums[rows, d]
        assert np.isfinite(p_sel).all() and not np.array_equal(p_sel, info.momentums[rows, (d + 1) % P])
        np.testing.assert_allclose(new.weights.astype(np.float64).sum(1), 1.0, rtol=0, atol=1e-6)
        np.testing.assert_allclose(info.weights_mean, 1.0 / P, rtol=0, atol=1e-6)
        np.testing.assert_allclose(info.weights_variance, new.weights.astype(np.float64).var(1), rtol=1e-5, atol=1e-9)
        assert np.array_equal(new.directions, st.directions) and new.weights.dtype == f32
        seen.update(ch.tolist())
        st = new
    assert len(seen) > 1 and seen != {0}  # the select is exercised

    def nan_on_far_rows(q):  # NaN on the half of the orbit's rows that moved farthest from the chain's start
        logp, g = fn(q)
        if q.shape[0] == N:
            return logp, g
        moved = np.abs(q - np.repeat(q0, P, axis=0)).max(axis=1)
        return np.where(moved > np.median(moved), f32(np.nan), logp).astype(f32), g

    st = ro.init(q0, fn, P)
    new, info, ch = ro.kernel(prng.key(7), st, nan_on_far_rows, eps, imm, P)
    nan_slots = np.isnan(new.logdensities)
    assert nan_slots.any() and not nan_slots.all(axis=1).any()
    assert not np.isnan(new.weights).any() and np.all(new.weights[nan_slots] == 0)
    np.testing.assert_allclose(new.weights.astype(np.float64).sum(1), 1.0, rtol=0, atol=1e-6)
    assert not np.isnan(info.weights_mean).any() and not np.isnan(info.weights_variance).any()


# |w P - 1| on this run: the exact flow conserves H, so the weights differ from 1 / P only by the fp32 rounding of
# H = -logp + kinetic energy (|H| up to ~20 here: ulp 2e-6) through exp.  The restatement's largest deviation over the 20
# transitions is 3.34e-6 (measured, this file's experiment as is); the bound is ten times that.
WEIGHT_BOUND = 3.4e-5


def test_orbital_restatement_is_stationary_on_the_exact_flow():
    """The periodic case: the exact flow of N(0, diag(sigma^2)) with step 2 pi / 8 closes the orbit of 8 slots.  2 048
    chains started at 3 sigma, 20 transitions: the across-chain averages of the weighted first and second moments of the
    last orbit lie within 5 standard errors (from the across-chain spread) of 0 and sigma^2, and every weight is 1 / P
    up to the rounding of the energy (WEIGHT_BOUND).  A float64 draft of this experiment gave |z| <= 1.7."""
    N, P, sigma, imm, q0, eps, keys = ro.exact_flow_case()
    fn = otargets.diag_gaussian((f32(1) / imm).astype(f32))
    flow = ro.gaussian_exact_flow(imm)
    st = ro.init(q0, fn, P)
    dev, seen = 0.0, set()
    for k in keys:
        st, info, ch = ro.kernel(k, st, fn, eps, imm, P, bijection=flow)
        dev = max(dev, float(np.abs(st.weights.astype(np.float64) * P - 1.0).max()))
        seen.update(ch.tolist())
    z = ro.weighted_moment_z_scores(st.positions, st.weights, sigma)
    print("largest |w P - 1|:", dev, " z scores:", z)
    assert dev <= WEIGHT_BOUND, dev
    assert np.all(np.abs(z) <= 5.0), z
    assert seen == set(range(P))  # every slot gets selected
