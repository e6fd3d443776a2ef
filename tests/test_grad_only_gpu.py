"""Gradient-only log-density launches inside an HMC trajectory (endpoint proposal: only the last evaluation's logp is
read) and evaluation into the driver's own buffers.  Nothing a transition returns may change: every comparison here is
``torch.equal``."""
import warnings

import pytest
import torch

import blackjax_amd as bjx
from blackjax_amd import _util, integrators
from test_device_target import QUARTIC

pytestmark = pytest.mark.gpu


def _rand(dev, seed, *shape):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randn(*shape, device=dev, generator=g)


def _diag(dev, D):
    return bjx.targets.DiagGaussian((0.5 + torch.rand(D, device=dev)).float())


def _grad_only_equals_full(tgt, q):
    lp, g = tgt(q)
    # evaluation into the caller's buffers: the same launch, other addresses
    lp2, g2 = torch.full_like(lp, float("nan")), torch.full_like(g, float("nan"))
    assert tgt._bjx_eval_into(q, lp2, g2) is not False
    assert torch.equal(lp, lp2) and torch.equal(g, g2)
    g3 = torch.full_like(g, float("nan"))
    assert tgt._bjx_grad_into(q, g3) is not False
    assert torch.equal(g, g3)
    # a slice of a larger array, as the driver hands over one chain block of its result arrays
    big = torch.full((q.shape[0] + 3, q.shape[1]), float("nan"), device=q.device)
    tgt._bjx_grad_into(q, big[2:2 + q.shape[0]])
    assert torch.equal(g, big[2:2 + q.shape[0]])
    assert bool(torch.isnan(big[:2]).all()) and bool(torch.isnan(big[2 + q.shape[0]:]).all())


@pytest.mark.parametrize("D", [7, 64, 100, 256, 1024, 2048])
@pytest.mark.parametrize("N", [1, 333, 4096])
def test_diag_gaussian_gradient_only_launch_has_the_bits_of_the_full_launch(dev, N, D):
    _grad_only_equals_full(_diag(dev, D), _rand(dev, 1000 * D + N, N, D))


def test_diag_gaussian_gradient_only_launch_above_the_infinity_cache_size(dev):
    """More than 256 MiB read + written in one launch: the nontemporal instantiations of both kernels."""
    N, D = 33024, 1024
    assert N * D * 8 > 256 << 20
    tgt, q = _diag(dev, D), _rand(dev, 5, N, D)
    lp, g = tgt(q)
    g2 = torch.full_like(g, float("nan"))
    tgt._bjx_grad_into(q, g2)
    assert torch.equal(g, g2)


def test_device_target_gradient_only_launch(dev):
    """A hand-written ``DeviceTarget`` holds rows of at most 1 024 floats: D = 256 (the D = 1 500 case is served by the
    generated row-loop target below)."""
    D = 256
    params = torch.cat([(0.5 + torch.rand(D, device=dev)).float(), torch.tensor([0.3], device=dev)]).contiguous()
    _grad_only_equals_full(bjx.targets.DeviceTarget(QUARTIC, params), _rand(dev, 11, 333, D))


@pytest.mark.parametrize("D", [256, 1500])
def test_from_elementwise_gradient_only_launch(dev, D):
    w = (0.5 + torch.rand(D, device=dev)).float()
    tgt = bjx.targets.from_elementwise(lambda q: -0.5 * (q * q * w).sum(-1) - torch.nn.functional.softplus(q).sum(-1),
                                       D, dev)
    assert type(tgt).__name__ == ("DeviceTarget" if D == 256 else "ElementwiseRowsTarget")
    _grad_only_equals_full(tgt, _rand(dev, 12, 333, D))


def _assert_same_transition(sa, ia, sb, ib):
    for x, y in zip(sa, sb):
        assert torch.equal(x, y)
    for name in ("momentum", "acceptance_rate", "is_accepted", "is_divergent", "energy"):
        assert torch.equal(getattr(ia, name), getattr(ib, name)), name
    for x, y in zip(ia.proposal, ib.proposal):
        assert torch.equal(x, y)
    assert ia.num_integration_steps == ib.num_integration_steps


@pytest.mark.parametrize("integrator", ["velocity_verlet", "mclachlan"])
@pytest.mark.parametrize("per_chain_eps", [False, True])
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("chain_block", [None, 0, 1024])
def test_transitions_equal_those_of_the_same_callable_without_capabilities(dev, chain_block, streams, use_graph,
                                                                           per_chain_eps, integrator):
    N, D, L = 2500, 256, 5
    tgt = _diag(dev, D)
    plain = bjx.returns_pair(lambda q: tgt(q))  # the same arithmetic; no in-place outputs, no gradient-only call
    assert getattr(_util.value_and_grad(plain), "_bjx_grad_into", None) is None
    imm = (0.5 + torch.rand(D, device=dev)).float()
    eps = (0.05 + 0.2 * torch.rand(N, device=dev)) if per_chain_eps else 0.11
    kw = dict(chain_block=chain_block, streams=streams, use_graph=use_graph,
              integrator=getattr(integrators, integrator))
    a, b = bjx.hmc(tgt, eps, imm, L, **kw), bjx.hmc(plain, eps, imm, L, **kw)
    q0 = _rand(dev, 21, N, D)
    sa, sb = a.init(q0), b.init(q0)
    for k in bjx.random.split(bjx.random.key(9), 3):
        sa, ia = a.step(k, sa)
        sb, ib = b.step(k, sb)
        _assert_same_transition(sa, ia, sb, ib)


@pytest.mark.parametrize("L", [1, 2])
def test_shortest_trajectories(dev, L):
    """L = 1: the only evaluation is the last one (full); L = 2: one gradient-only call, one full."""
    N, D = 300, 1024
    tgt = _diag(dev, D)
    plain = bjx.returns_pair(lambda q: tgt(q))
    imm = torch.ones(D, device=dev)
    q0 = _rand(dev, 3, N, D)
    for kw in (dict(), dict(chain_block=128), dict(use_graph=True)):
        a, b = bjx.hmc(tgt, 0.05, imm, L, **kw), bjx.hmc(plain, 0.05, imm, L, **kw)
        sa, sb = a.init(q0), b.init(q0)
        for k in bjx.random.split(bjx.random.key(1), 2):
            sa, ia = a.step(k, sa)
            sb, ib = b.step(k, sb)
            _assert_same_transition(sa, ia, sb, ib)


@pytest.mark.parametrize("chain_block,n_blocks", [(0, 1), (1024, 3)])
def test_a_plain_callable_is_called_exactly_as_before(dev, chain_block, n_blocks):
    """A callable without the capabilities: L calls per block per transition, each on the block's (n, D) positions."""
    N, D, L = 2500, 64, 6
    seen = []

    def fn(q):
        seen.append(tuple(q.shape))
        return -0.5 * (q * q).sum(-1), -q

    alg = bjx.hmc(bjx.returns_pair(fn), 0.1, torch.ones(D, device=dev), L, chain_block=chain_block)
    state = alg.init(_rand(dev, 4, N, D))
    assert seen == [(N, D)]
    for k in bjx.random.split(bjx.random.key(2), 2):
        del seen[:]
        state, info = alg.step(k, state)
        blocks = [(min(1024, N - 1024 * b) if chain_block else N, D) for b in range(n_blocks)]
        assert seen == [s for s in blocks for _ in range(L)]


def test_a_stale_traced_function_is_caught_when_only_gradient_only_calls_came_in_between(dev):
    """The re-check of a traced function (kernel call 16) counts gradient-only calls and compares the full
    (logp, grad) with autograd when its turn comes."""
    box = {"beta": 1.0}

    def tempered(q):
        return -0.5 * box["beta"] * (q * q).sum(-1)

    q = _rand(dev, 6, 32, 16)
    vg = _util.value_and_grad(tempered)
    vg(q)                                        # first call: autograd, then traced with beta = 1
    assert list(vg._bjx_elementwise.values())[0] is not None
    box["beta"] = 3.0
    g = torch.empty_like(q)
    for _ in range(15):                          # kernel calls 1 .. 15, all gradient-only
        assert _util.eval_into(vg, q, None, g, need_logp=False)[1] is g
        assert torch.allclose(g, -q)
    with pytest.warns(RuntimeWarning, match="no longer agrees"):
        lp, g16 = _util.eval_into(vg, q, None, g, need_logp=False)   # call 16: declined, re-checked in full
    assert g16 is not g and torch.allclose(g16, -3.0 * q) and torch.allclose(lp, -1.5 * (q * q).sum(-1))
    assert list(vg._bjx_elementwise.values())[0] is None
    lp, g17 = _util.eval_into(vg, q, None, g, need_logp=False)       # eager autograd from here on
    assert g17 is not g and torch.allclose(g17, -3.0 * q)


def test_a_traced_function_takes_the_gradient_only_path_and_keeps_its_results(dev):
    """``hmc`` on a plain PyTorch function: the transitions of the traced function (gradient-only launches, in-place
    outputs) equal those driven through its generated target hidden behind ``returns_pair``."""
    N, D, L = 700, 256, 5
    w = (0.5 + torch.rand(D, device=dev)).float()

    def fn(q):
        return -0.5 * (q * q * w).sum(-1)

    hidden_tgt = bjx.targets.from_elementwise(fn, D, dev)
    hidden = bjx.returns_pair(lambda q: hidden_tgt(q))
    imm = torch.ones(D, device=dev)
    q0 = _rand(dev, 8, N, D)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (small launches from Python: announced once)
        a, b = bjx.hmc(fn, 0.1, imm, L, chain_block=256), bjx.hmc(hidden, 0.1, imm, L, chain_block=256)
        a.init(q0)  # the first call of a plain function is served by autograd (and traces it): its logp has other bits
        sa = sb = b.init(q0)
        for k in bjx.random.split(bjx.random.key(5), 4):  # 60 kernel calls: past the re-check at call 16
            sa, ia = a.step(k, sa)
            sb, ib = b.step(k, sb)
            _assert_same_transition(sa, ia, sb, ib)
    assert list(_util.value_and_grad(fn)._bjx_elementwise.values())[0] is not None
