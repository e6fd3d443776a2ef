"""Store policy of the cache-resident HMC loop kernels (flat leapfrog, gradient-only Gaussian callable): p, q and g are
written through L2 with buffer stores (``st4_wt``, csrc/bjx_device.h).  Only where the bytes go changes, so every
comparison here is exact equality with the oracle's fp32 restatement of the same stage (``oracle.fp.fma32``, the
arithmetic of ``oracle.hmc.velocity_verlet``).

Shapes: the smallest at which the changed code can still go wrong -- whole groups of eight workgroups (24 x 1 024), an
unaligned last group with two workgroups per row (9 x 2 048), and the any-row-length kernels with a ragged last
workgroup, whose buffer descriptor ends with the arrays (1 000 x 8, 37 x 100)."""
import numpy as np
import pytest
import torch

import blackjax_amd as bjx
from blackjax_amd import _lib
from oracle import hmc as ohmc
from oracle import targets as otargets
from oracle.fp import f32, fma32

pytestmark = pytest.mark.gpu

SHAPES = [(24, 1024), (9, 2048), (1000, 8), (37, 100)]


def t2n(t):
    return t.detach().cpu().numpy()


def dev_t(a, dev):
    return torch.as_tensor(np.asarray(a), device=dev)


def _stage(q, p, g, eps, imm, kicks):
    """One launch of the leapfrog kernel: ``kicks`` half kicks, then the drift (velocity_verlet's lines, in its order)."""
    eps = np.asarray(eps, f32)[:, None] if np.ndim(eps) else f32(eps)
    h = (eps * f32(0.5)).astype(f32) if np.ndim(eps) else f32(eps * f32(0.5))
    for _ in range(kicks):
        p = fma32(h, g, p)
    return fma32(eps, (imm * p).astype(f32), q), p


def _inputs(N, D, per_chain_eps, per_chain_imm, seed):
    rng = np.random.default_rng(seed)
    q, p = (rng.standard_normal((N, D)).astype(np.float32) for _ in range(2))
    imm = rng.uniform(0.1, 4.0, size=(N, D) if per_chain_imm else (D,)).astype(np.float32)
    eps = rng.uniform(0.01, 0.3, size=N).astype(np.float32) if per_chain_eps else np.float32(0.1)
    inv_var = rng.uniform(0.5, 2.0, size=D).astype(np.float32)
    return q, p, imm, eps, inv_var


@pytest.mark.parametrize("per_chain_imm", [False, True])
@pytest.mark.parametrize("per_chain_eps", [False, True])
@pytest.mark.parametrize("N,D", SHAPES)
def test_leapfrog_and_gradient_launches_have_the_oracles_bits(dev, N, D, per_chain_eps, per_chain_imm):
    """One kick out of place, the gradient-only callable, two kicks in place, and the masked entry point out of place
    and in place with some chains finished: q, p and g equal the oracle's, element for element."""
    q, p, imm, eps, inv_var = _inputs(N, D, per_chain_eps, per_chain_imm, 1)
    fn = otargets.diag_gaussian(inv_var)
    _, g = fn(q)
    q1, p1 = _stage(q, p, g, eps, imm, 1)
    # the restatement IS the oracle's integrator: its position after one step
    z1 = ohmc.velocity_verlet(ohmc.IntegratorState(q, p, None, g), eps, fn, ohmc.default_metric(imm, n_chains=N))
    assert np.array_equal(q1, z1.position)
    _, g1 = fn(q1)
    q2, p2 = _stage(q1, p1, g1, eps, imm, 2)

    qt, pt, gt, immt, ivt = (dev_t(a, dev) for a in (q, p, g, imm, inv_var))
    eps_pc = dev_t(eps, dev) if per_chain_eps else None
    s = _lib.current_stream()
    head = lambda kicks: (s, N, D, kicks, 0.0 if per_chain_eps else float(eps), _lib.ptr(eps_pc), immt.data_ptr(),
                          D if per_chain_imm else 0)
    qo, po = torch.full_like(qt, float("nan")), torch.full_like(pt, float("nan"))
    _lib.call("bjx_leapfrog_diag", *head(1), qt.data_ptr(), pt.data_ptr(), gt.data_ptr(), qo.data_ptr(), po.data_ptr())
    assert np.array_equal(t2n(qo), q1) and np.array_equal(t2n(po), p1)
    assert np.array_equal(t2n(qt), q) and np.array_equal(t2n(pt), p)  # out of place: the inputs stay
    go = torch.full_like(gt, float("nan"))
    _lib.call("bjx_target_diag_gaussian_grad", s, N, D, ivt.data_ptr(), qo.data_ptr(), go.data_ptr())
    assert np.array_equal(t2n(go), g1)
    _lib.call("bjx_leapfrog_diag", *head(2), qo.data_ptr(), po.data_ptr(), go.data_ptr(), qo.data_ptr(), po.data_ptr())
    assert np.array_equal(t2n(qo), q2) and np.array_equal(t2n(po), p2)

    # masked entry point: chains with step_idx >= n_steps are copied through (out of place) or left alone (in place)
    n_steps = np.array([(i * 2) % 5 for i in range(N)], np.int32)
    step_idx = 2
    live = (n_steps > step_idx)[:, None]
    for kicks, (qs, ps) in ((1, (q1, p1)), (2, (q2, p2))):
        q_in, p_in, g_in = (q, p, g) if kicks == 1 else (q1, p1, g1)
        want_q, want_p = np.where(live, qs, q_in), np.where(live, ps, p_in)
        a, b, c, nst = (dev_t(x, dev) for x in (q_in, p_in, g_in, n_steps))
        qm, pm = torch.full_like(a, float("nan")), torch.full_like(b, float("nan"))
        _lib.call("bjx_leapfrog_diag_masked", *head(kicks), a.data_ptr(), b.data_ptr(), c.data_ptr(), qm.data_ptr(),
                  pm.data_ptr(), nst.data_ptr(), step_idx)
        assert np.array_equal(t2n(qm), want_q) and np.array_equal(t2n(pm), want_p)
        _lib.call("bjx_leapfrog_diag_masked", *head(kicks), a.data_ptr(), b.data_ptr(), c.data_ptr(), a.data_ptr(),
                  b.data_ptr(), nst.data_ptr(), step_idx)
        assert np.array_equal(t2n(a), want_q) and np.array_equal(t2n(b), want_p)


def test_alternating_loop_in_place_reads_no_stale_line(dev):
    """Eight trajectory steps as the driver issues them -- leapfrog in place, gradient into g, nothing in between --
    at 64 x 1 024: a launch that read a line its predecessor's store left stale in some L2 would miss the oracle."""
    N, D, L = 64, 1024, 8
    q, p, imm, eps, inv_var = _inputs(N, D, False, False, 2)
    fn = otargets.diag_gaussian(inv_var)
    _, g = fn(q)
    qt, pt, gt, immt, ivt = (dev_t(a, dev) for a in (q, p, g, imm, inv_var))
    s = _lib.current_stream()
    for k in range(L):
        _lib.call("bjx_leapfrog_diag", s, N, D, 1 if k == 0 else 2, float(eps), None, immt.data_ptr(), 0, qt.data_ptr(),
                  pt.data_ptr(), gt.data_ptr(), qt.data_ptr(), pt.data_ptr())
        _lib.call("bjx_target_diag_gaussian_grad", s, N, D, ivt.data_ptr(), qt.data_ptr(), gt.data_ptr())
    z = ohmc.IntegratorState(q, p, None, g)
    metric = ohmc.default_metric(imm, n_chains=N)
    for _ in range(L):
        z = ohmc.velocity_verlet(z, eps, fn, metric)
    assert np.array_equal(t2n(qt), z.position)
    assert np.array_equal(t2n(gt), z.logdensity_grad)
    # the device holds the momentum before the closing half kick
    assert np.array_equal(fma32(f32(eps * f32(0.5)), z.logdensity_grad, t2n(pt)), z.momentum)


def _assert_equal_fields(a, b, path):
    if isinstance(a, torch.Tensor):
        assert torch.equal(a, b), path
    elif isinstance(a, tuple):
        assert len(a) == len(b), path
        for name, x, y in zip(getattr(a, "_fields", range(len(a))), a, b):
            _assert_equal_fields(x, y, f"{path}.{name}")
    else:
        assert a == b, path


def test_blocked_transitions_equal_one_launch_transitions(dev):
    """``hmc(...).step``, three transitions at 40 x 1 024: cache blocks of 16 chains (a ragged last block of 8; the
    opening kick, the loop and the last full evaluation per block) against one launch per stage."""
    N, D, L = 40, 1024, 4
    g_ = torch.Generator(device=dev)
    g_.manual_seed(7)
    tgt = bjx.targets.DiagGaussian((0.5 + torch.rand(D, device=dev, generator=g_)).float())
    imm = (0.5 + torch.rand(D, device=dev, generator=g_)).float()
    q0 = torch.randn(N, D, device=dev, generator=g_)
    a, b = bjx.hmc(tgt, 0.11, imm, L, chain_block=16), bjx.hmc(tgt, 0.11, imm, L, chain_block=0)
    sa, sb = a.init(q0), b.init(q0)
    for k in bjx.random.split(bjx.random.key(3), 3):
        sa, ia = a.step(k, sa)
        sb, ib = b.step(k, sb)
        _assert_equal_fields(sa, sb, "state")
        _assert_equal_fields(ia, ib, "info")
