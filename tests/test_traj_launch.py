"""Which entry point of libbjxhip each operation of ``_traj_launch.Launcher`` launches, and that every argument fits the
ctypes prototype: needs no GPU (CPU tensors, ``_lib.call`` replaced by a recorder -- the launcher only reads
``data_ptr()``, shapes and the metric's ``kind``).  The expected names are written out per call site (sampler x
metric x integrator x per-chain lengths), not derived from the launcher's own flags."""
import ctypes
import itertools

import pytest
import torch

from blackjax_amd import _lib, _traj_launch, integrators
from blackjax_amd.metrics import Metric

N, D = 6, 4
VV, THREE_STAGE = integrators.velocity_verlet, integrators.yoshida
KEY, OFF, STREAM, EPS, THR = (11, 22, 5), 3, 0x1000, 0.1, 1000.0


def _metric(kind):
    eye = torch.eye(D)
    if kind == "diag":
        return Metric("diag", torch.ones(D), 0, None)
    if kind == "diag_pc":
        return Metric("diag", torch.ones(N, D), D, None)
    if kind == "dense":
        return Metric("dense", eye.clone(), 0, eye.clone(), eye.clone())
    stack = eye.expand(N, D, D).contiguous()
    return Metric("dense_pc", stack, 0, stack.clone(), None)


KINDS = ["diag", "diag_pc", "dense", "dense_pc"]
SUFFIX = {"dense": "dense", "dense_pc": "dense_pc"}


def expected_stage(sampler, kind, general, lengths):
    if kind.startswith("diag"):
        if sampler == "dmhmc" or general:
            return "bjx_leapfrog_diag_coef"
        return "bjx_leapfrog_diag_masked" if lengths else "bjx_leapfrog_diag"  # (lengths: dynamic_hmc only)
    if general or sampler in ("dynamic_hmc", "dmhmc"):
        return "bjx_leapfrog_dense_coef"
    return "bjx_leapfrog_" + SUFFIX[kind]


def expected_finish(kind, general):
    if kind.startswith("diag"):
        return "bjx_hmc_finish_diag_coef" if general else "bjx_hmc_finish_diag"
    return "bjx_hmc_finish_dense_coef" if general else "bjx_hmc_finish_" + SUFFIX[kind]


def expected_mhmc_step(sampler, kind, general):
    if kind.startswith("diag"):
        return "bjx_mhmc_step_diag_coef" if (general or sampler == "dmhmc") else "bjx_mhmc_step_diag"
    if general:
        return "bjx_mhmc_step_dense_coef"
    return "bjx_mhmc_step_dense_masked" if sampler == "dmhmc" else "bjx_mhmc_step_dense"


@pytest.fixture
def calls(monkeypatch):
    rec = []

    def record(name, *args):
        _check_prototype(name, args)
        rec.append((name, args))

    monkeypatch.setattr(_lib, "call", record)
    return rec


def _check_prototype(name, args):
    sig = _lib.SIGNATURES[name]
    assert len(args) == len(sig), (name, len(args), len(sig))
    for i, (t, a) in enumerate(zip(sig, args)):
        if t is ctypes.c_void_p:
            ok = a is None or type(a) is int
        elif t is ctypes.c_float:
            ok = type(a) is float
        else:
            assert t in (ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32), (name, i, t)
            ok = type(a) is int  # neither bool nor a tensor
        assert ok, f"{name}: argument {i} = {a!r} does not fit {t.__name__}"


def _launcher(sampler, kind, integrator):
    c = integrator.coefficients
    return _traj_launch.Launcher(_metric(kind), c[0::2], c[1::2], integrator is not VV, sampler)


def _mat():
    return torch.zeros(N, D)


def _vec(dtype=torch.float32):
    return torch.zeros(N, dtype=dtype)


CASES = [(s, k, i, n) for s, k, i, n in itertools.product(("hmc", "mhmc", "dynamic_hmc", "dmhmc"), KINDS,
                                                          (VV, THREE_STAGE), (False, True))
         if not (n and s in ("hmc", "mhmc"))]  # the static samplers never pass lengths


@pytest.mark.parametrize("sampler,kind,integrator,lengths", CASES,
                         ids=[f"{s}-{k}-{i}-{'lengths' if n else 'nolengths'}" for s, k, i, n in CASES])
@pytest.mark.parametrize("eps_pc", [False, True], ids=["eps", "eps_pc"])
def test_every_operation_launches_its_entry_point_with_arguments_that_fit(calls, sampler, kind, integrator, lengths,
                                                                          eps_pc):
    lau = _launcher(sampler, kind, integrator)
    general = integrator is not VV
    n_steps = _vec(torch.int32) if lengths else None
    eps, epc = (0.0, _vec()) if eps_pc else (EPS, None)
    p0, ke0 = _mat(), _vec()

    lau.momentum(STREAM, KEY, OFF, N, D, p0, ke0)
    assert [c[0] for c in calls] == ["bjx_hmc_momentum_" + ("diag" if kind.startswith("diag") else SUFFIX[kind])]
    if kind.startswith("diag"):
        lau.momentum_kick(STREAM, KEY, OFF, N, D, eps, epc, _mat(), _mat(), p0, ke0, _mat(), _mat())
        assert calls[-1][0] == "bjx_hmc_momentum_kick_diag"
    assert bool(lau.fuses_first(132)) == (kind.startswith("diag") and not general and _traj_launch._FUSE_FIRST)
    assert not lau.fuses_first(128)

    # every position update of a two-step trajectory, then a masked / unmasked single stage with p_out left to stage()
    del calls[:]
    q, p, g = _mat(), _mat(), _mat()
    for step, _, n_kicks, ka, kb, a in lau.updates(2):
        p = lau.stage(STREAM, N, D, n_kicks, ka, kb, a, eps, epc, q, p, g, q, p, n_steps, step)
        assert p.shape == (N, D)
    p2 = lau.stage(STREAM, N, D, 1, 0.5, 0.0, 1.0, eps, epc, q, p, g, q, None, n_steps, 1)
    assert (p2 is p) == kind.startswith("diag")  # in place where the kernel can, else a fresh buffer
    assert len(calls) == 2 * len(integrator.coefficients[1::2]) + 1
    assert {c[0] for c in calls} == {expected_stage(sampler, kind, general, lengths)}
    if calls[0][0].endswith("_coef"):  # (stream, n, d, n_kicks, ka, kb, a, ...)
        b, a = integrator.coefficients[0::2], integrator.coefficients[1::2]
        assert calls[0][1][3:7] == (1, b[0], 0.0, a[0])
        assert calls[1][1][3:7] == ((1, b[1], 0.0, a[1]) if general else (2, 0.5, 0.5, 1.0))
        assert calls[-1][1][-2:] == (_lib.ptr(n_steps), 1)

    if sampler in ("hmc", "dynamic_hmc"):
        del calls[:]
        lau.finish(STREAM, KEY, OFF, N, D, eps, epc, THR, _mat(), _vec(), _mat(), _vec(), q, _vec(), g, p, _mat(),
                   _mat(), _vec(), _mat(), _vec(), _vec(torch.bool), _vec(torch.bool), _vec())
        assert [c[0] for c in calls] == [expected_finish(kind, general)]
    else:
        acc = (_vec(), _vec(), _vec(torch.bool), _vec(torch.bool), _mat(), _mat(), _mat(), _vec(), _vec())
        steps = _vec(torch.int32) if sampler == "dmhmc" else None  # (its opening stage alone passes no lengths)
        for reopen in (False, True):
            del calls[:]
            p_next = lau.mhmc_step(STREAM, KEY, OFF, N, D, 1, reopen, eps, epc, THR, _vec(), _vec(), q, p, g, _vec(),
                                   *acc, n_steps=steps)
            assert p_next.shape == (N, D)
            names = [c[0] for c in calls]
            if kind.startswith("diag"):  # the re-opening is fused: one launch, flag 0 / 1
                assert names == [expected_mhmc_step(sampler, kind, general)] and calls[0][1][8] == int(reopen)
                assert p_next is p
            else:                        # a step, then a leapfrog launch from the fully kicked momentum
                assert names == [expected_mhmc_step(sampler, kind, general)] + (
                    [expected_stage(sampler, kind, general, lengths)] if reopen else [])
                if reopen and names[1].endswith("_coef"):
                    assert calls[1][1][-1] == (2 if steps is not None else 0)  # masked by lengths at step + 1
        del calls[:]
        lau.mhmc_finish(STREAM, N, D, 2, steps, _mat(), _mat(), _mat(), _vec(), _vec(), _vec(torch.bool), _vec(),
                        _mat(), _mat(), _mat(), _vec(), _vec(), _vec())
        assert [c[0] for c in calls] == ["bjx_mhmc_finish_masked" if steps is not None else "bjx_mhmc_finish"]


def test_position_updates_of_a_trajectory():
    """Opening kick b1 once, then per step the merged closing + opening kicks; stages 2 .. K are single kicks."""
    assert list(_launcher("hmc", "diag", VV).updates(3)) == [
        (0, 0, 1, 0.5, 0.0, 1.0), (1, 0, 2, 0.5, 0.5, 1.0), (2, 0, 2, 0.5, 0.5, 1.0)]
    b, a = THREE_STAGE.coefficients[0::2], THREE_STAGE.coefficients[1::2]
    assert list(_launcher("hmc", "diag", THREE_STAGE).updates(2)) == [
        (0, 0, 1, b[0], 0.0, a[0]), (0, 1, 1, b[1], 0.0, a[1]), (0, 2, 1, b[2], 0.0, a[2]),
        (1, 0, 2, b[3], b[0], a[0]), (1, 1, 1, b[1], 0.0, a[1]), (1, 2, 1, b[2], 0.0, a[2])]
    assert list(_launcher("hmc", "diag", VV).updates(0)) == []


def test_shared_dense_matrix_pointer_follows_the_rows_of_the_launch(calls):
    """Whole 128 x 128 tiles read the matrix as stored, ragged launches its transposed copy: decided by the rows of
    the launch (a chain block), not of the batch."""
    d = 128
    m = Metric("dense", torch.eye(d), 0, torch.eye(d), torch.eye(d))
    lau = _traj_launch.Launcher(m).rows(slice(0, 128))
    for n in (128, 44):
        x = torch.zeros(n, d)
        lau.stage(STREAM, n, d, 1, 0.5, 0.0, 1.0, EPS, None, x, x, x, x, torch.zeros(n, d))
    assert [c[0] for c in calls] == ["bjx_leapfrog_dense"] * 2
    assert [c[1][6] for c in calls] == [m.imm.data_ptr(), m.imm_t.data_ptr()]


def test_a_chain_block_takes_its_rows_of_per_chain_matrices():
    for kind in KINDS:
        lau = _launcher("hmc", kind, VV)
        blk = lau.rows(slice(2, 5))
        m, mb = lau.metric, blk.metric
        if kind in ("diag_pc", "dense_pc"):
            assert mb.imm.shape[0] == 3 and mb.imm.data_ptr() == m.imm[2:5].data_ptr()
        else:
            assert mb.imm.data_ptr() == m.imm.data_ptr()
        if kind == "dense_pc":
            assert mb.mass_sqrt_t.data_ptr() == m.mass_sqrt_t[2:5].data_ptr()
        assert (blk.general, blk.sampler, blk.kick_c, blk.drift_c) == (lau.general, lau.sampler, lau.kick_c,
                                                                       lau.drift_c)
