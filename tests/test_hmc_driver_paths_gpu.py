"""Every host path of the HMC driver gives the same transition, bit for bit: one launch over all chains against
chain blocks, blocks on two streams and the graphed block loop, for every metric kind, velocity Verlet and a
three-stage integrator.  ``L = 3`` has the opening one-kick launch, a two-kick launch and the closing kick; N = 300 in
blocks of 128 is 128 / 128 / 44 rows, so the shared dense matrix runs on whole 128 x 128 tiles (D = 128, full blocks)
and on the ragged kernel (the 44-row block, the unblocked batch, D = 132)."""
import functools

import pytest
import torch

import blackjax_amd as bjx
from blackjax_amd import integrators

pytestmark = pytest.mark.gpu

N, EPS = 300, 0.1
METRICS = {"diag": 132, "diag_pc": 132, "dense128": 128, "dense132": 132, "dense_pc": 24}
BLOCKED = [dict(chain_block=128), dict(chain_block=128, streams=2)]
GRAPHED = dict(use_graph=True, chain_block=128)


def _randn(seed, *shape):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randn(*shape, generator=g)


@functools.lru_cache(maxsize=None)
def _problem(kind):
    """-> (target, inverse mass matrix, initial positions): a Gaussian with a fixed scale per coordinate."""
    dev = torch.device("cuda:0")
    D = METRICS[kind]
    tgt = bjx.targets.DiagGaussian(torch.linspace(0.5, 2.0, D, device=dev))
    if kind == "diag":
        imm = torch.linspace(0.6, 1.7, D)
    elif kind == "diag_pc":
        imm = 0.5 + torch.rand(N, D, generator=torch.Generator().manual_seed(3))
    else:
        a = _randn(4, *((N, D, D) if kind == "dense_pc" else (D, D)))
        imm = a @ a.transpose(-1, -2) / D + torch.eye(D)
    return tgt, imm.to(dev).contiguous(), _randn(5, N, D).to(dev)


@functools.lru_cache(maxsize=None)
def _transition(sampler, kind, integrator, L, per_chain_eps=False, **kw):
    tgt, imm, q0 = _problem(kind)
    eps = torch.full((N,), EPS, device=q0.device) if per_chain_eps else EPS
    alg = getattr(bjx, sampler)(tgt, eps, imm, L, integrator=getattr(integrators, integrator), **kw)
    return alg.step(bjx.random.key(7), alg.init(q0))


def _assert_same_transition(a, b):
    (sa, ia), (sb, ib) = a, b
    for name in sa._fields:
        assert torch.equal(getattr(sa, name), getattr(sb, name)), name
    for name in ("momentum", "acceptance_rate", "is_accepted", "is_divergent", "energy"):
        assert torch.equal(getattr(ia, name), getattr(ib, name)), name
    for name in ia.proposal._fields:
        assert torch.equal(getattr(ia.proposal, name), getattr(ib.proposal, name)), "proposal." + name
    assert ia.num_integration_steps == ib.num_integration_steps
    assert bool(torch.isfinite(sa.position).all()) and bool(torch.isfinite(ia.energy).all())


def _hmc_cases():
    for kind in METRICS:
        for integrator in ("velocity_verlet", "mclachlan"):
            for L in (3, 0, 1) if kind.startswith("diag") else (3,):
                paths = BLOCKED + ([GRAPHED] if kind.startswith("diag") and integrator == "velocity_verlet" else [])
                for kw in paths:
                    yield pytest.param(kind, integrator, L, kw,
                                       id="-".join([kind, integrator, f"L{L}"] + [f"{k}={v}" for k, v in kw.items()]))


@pytest.mark.parametrize("kind,integrator,L,kw", list(_hmc_cases()))
def test_hmc_transition_is_the_same_on_every_host_path(dev, kind, integrator, L, kw):
    one_launch = _transition("hmc", kind, integrator, L, chain_block=0)
    _assert_same_transition(one_launch, _transition("hmc", kind, integrator, L, **kw))


@pytest.mark.parametrize("integrator", ["velocity_verlet", "mclachlan"])
@pytest.mark.parametrize("kind", list(METRICS))
def test_mhmc_transition_with_a_per_chain_step_size_filled_with_the_scalar(dev, kind, integrator):
    """``chain_block`` does not apply to the multinomial proposal: its one host path per metric and integrator is run
    with the scalar step size and with an ``(N,)`` tensor holding that value."""
    _assert_same_transition(_transition("mhmc", kind, integrator, 3),
                            _transition("mhmc", kind, integrator, 3, per_chain_eps=True))
