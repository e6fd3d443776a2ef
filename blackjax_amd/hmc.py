"""Batched HMC on MI355X behind the ``blackjax.hmc`` API surface.

Mirrors blackjax/mcmc/hmc.py: ``HMCState`` (38-49), ``HMCInfo`` (52-87), ``init``
(90-92), ``build_kernel`` (251-314), ``as_top_level_api`` (317-414).  The chain
axis is native: every field carries a leading ``N``; chain ``i`` of
``step(rng_key, state)`` reproduces the reference's single-chain
``step(jax.random.split(rng_key, N)[i], state_i)`` (the vmap layout of
docs/examples/howto_sample_multiple_chains.md:120-127).

The arithmetic runs in libbjxhip's HIP kernels (include/bjx_hip.h); this module
only sequences launches around the user's PyTorch log-density callable.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional

import torch

from . import _lib, integrators, metrics
from ._util import (new_graph, record_graph, check_batch, eval_into, eval_logdensity, is_capturable, step_size_args,
                    value_and_grad, warn_eager_driver)
from ._traj_launch import Launcher
from .base import SamplingAlgorithm
from .random import key_spec

__all__ = ["HMCState", "HMCInfo", "IntegratorState", "init", "flip_momentum", "build_kernel", "as_top_level_api"]


class HMCState(NamedTuple):
    """blackjax/mcmc/hmc.py:38-49, batched: (N, D), (N,), (N, D)."""

    position: torch.Tensor
    logdensity: torch.Tensor
    logdensity_grad: torch.Tensor


class IntegratorState(NamedTuple):
    """blackjax/mcmc/integrators.py:43-53, batched."""

    position: torch.Tensor
    momentum: torch.Tensor
    logdensity: torch.Tensor
    logdensity_grad: torch.Tensor


class HMCInfo(NamedTuple):
    """blackjax/mcmc/hmc.py:52-87, batched."""

    momentum: torch.Tensor
    acceptance_rate: torch.Tensor
    is_accepted: torch.Tensor
    is_divergent: torch.Tensor
    energy: torch.Tensor
    proposal: IntegratorState
    num_integration_steps: int


def flip_momentum(state: IntegratorState) -> IntegratorState:
    """blackjax/mcmc/hmc.py:95-112: the end state of a trajectory with its momentum negated (time reversibility).  The
    transition kernels do this inside their finishing launch (``k_hmc_finish_*``: the flipped momentum is what ``HMCInfo.
    proposal`` carries); this is the stand-alone function of the reference for code that builds on it."""
    return IntegratorState(state.position, -1.0 * state.momentum, state.logdensity, state.logdensity_grad)


def init(position: torch.Tensor, logdensity_fn: Callable) -> HMCState:
    """blackjax/mcmc/hmc.py:90-92."""
    position = check_batch(position, "position")
    if position.ndim != 2:
        raise ValueError(f"position must be (n_chains, dim), got {tuple(position.shape)}")
    logp, grad = eval_logdensity(value_and_grad(logdensity_fn), position)
    return HMCState(position, logp, grad)


class _ProposalKind:
    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return self.name


#: selectors for ``build_kernel(build_proposal=...)`` (blackjax/mcmc/hmc.py:115-178, 181-248)
hmc_proposal = _ProposalKind("hmc_proposal")
multinomial_hmc_proposal = _ProposalKind("multinomial_hmc_proposal")


def _prologue(rng_key, state, logdensity_fn, step_size, inverse_mass_matrix, chain_offset):
    """The validated inputs of one transition: ``q0, logp0, g0, N, D, key, vg, metric, eps, eps_pc, stream, off``
    (``key`` = ``key_spec``'s (k0, k1, fold); ``eps, eps_pc`` = ``step_size_args``')."""
    q0 = check_batch(state.position, "state.position")
    logp0 = check_batch(state.logdensity, "state.logdensity")
    g0 = check_batch(state.logdensity_grad, "state.logdensity_grad")
    N, D = q0.shape
    metric = metrics.default_metric(inverse_mass_matrix, N, D, q0.device)
    eps, eps_pc = step_size_args(step_size, N, q0.device)
    return (q0, logp0, g0, N, D, key_spec(rng_key), value_and_grad(logdensity_fn), metric, eps, eps_pc,
            _lib.current_stream(), int(chain_offset))


def _multinomial_transition(thr, kick_c, drift_c, rng_key, state, logdensity_fn, step_size, inverse_mass_matrix, L,
                            chain_offset=0, draw_steps=None):
    """blackjax.mhmc / dmhmc: ``build_kernel(build_proposal=multinomial_hmc_proposal)`` (hmc.py:181-248 with
    trajectory.static_progressive_integration 170-232).  Instead of the trajectory end point, one
    state of the whole trajectory is drawn proportionally to exp(-H) by progressive (reservoir)
    sampling; there is no Metropolis rejection (``is_accepted`` is always True).  ``draw_steps(device)`` (dmhmc; called
    once the inputs are validated) returns per-chain trajectory lengths ``(n_steps, shortest, longest)``: ``L`` is then
    the longest, every launch after the opening one is masked by them, and finished chains keep their q, so the
    callable returns the same (logp, g) for them again, unused.

    Any palindromic integrator [b1, a1, ..., b1] (integrators.py:104-150): a step is closed with (eps b1) g and the
    next one opened with (eps b1) g, (eps a1) M^{-1} p (``Launcher.mhmc_step``: one launch with a diagonal metric; with
    a dense one the next leapfrog starts from the fully kicked momentum with its own, separately rounded, opening
    kick); the stages in between are plain kick + drift launches, each followed by the callable."""
    q0, logp0, g0, N, D, key, vg, metric, eps, eps_pc, stream, off = _prologue(
        rng_key, state, logdensity_fn, step_size, inverse_mass_matrix, chain_offset)
    dev = q0.device
    n_steps = None
    if draw_steps is not None:
        n_steps, _, L = draw_steps(dev)
    general = tuple(kick_c) != (0.5, 0.5) or tuple(drift_c) != (1.0,)
    lau = Launcher(metric, kick_c, drift_c, general, "mhmc" if n_steps is None else "dmhmc")
    p0 = torch.empty_like(q0)
    ke0 = torch.empty_like(logp0)
    lau.momentum(stream, key, off, N, D, p0, ke0)
    weight = torch.zeros_like(logp0)
    slpa = torch.full_like(logp0, float("-inf"))
    any_div = torch.zeros(N, dtype=torch.bool, device=dev)
    ever = torch.zeros(N, dtype=torch.bool, device=dev)
    pq, pp, pg = torch.empty_like(q0), torch.empty_like(q0), torch.empty_like(q0)
    plogp, penergy, acc_rate = torch.empty_like(logp0), torch.empty_like(logp0), torch.empty_like(logp0)
    if L > 0:
        q = torch.empty_like(q0)
        p = lau.stage(stream, N, D, 1, lau.kick_c[0], 0.0, lau.drift_c[0], eps, eps_pc, q0, p0, g0, q,
                      torch.empty_like(q0))
    for i in range(L):
        logp, g = eval_logdensity(vg, q)
        for si in range(1, len(lau.drift_c)):  # stages 2 .. K
            p = lau.stage(stream, N, D, 1, lau.kick_c[si], 0.0, lau.drift_c[si], eps, eps_pc, q, p, g, q, None,
                          n_steps, 0 if n_steps is None else i)
            logp, g = eval_logdensity(vg, q)
        p = lau.mhmc_step(stream, key, off, N, D, i, i + 1 < L, eps, eps_pc, thr, logp0, ke0, q, p, g, logp, weight,
                          slpa, any_div, ever, pq, pp, pg, plogp, penergy, n_steps=n_steps)
    lau.mhmc_finish(stream, N, D, L, n_steps, q0, p0, g0, logp0, ke0, ever, slpa, pq, pp, pg, plogp, penergy, acc_rate)
    info = HMCInfo(p0, acc_rate, torch.ones(N, dtype=torch.bool, device=dev), any_div, penergy,
                   IntegratorState(pq, pp, plogp, pg), L if n_steps is None else n_steps)
    return HMCState(pq, plogp, pg), info


def _build_mhmc_kernel(thr: float, kick_c=(0.5, 0.5), drift_c=(1.0,)):
    def kernel(rng_key, state: HMCState, logdensity_fn: Callable, step_size,
               inverse_mass_matrix, num_integration_steps: int, *, chain_offset: int = 0):
        L = int(num_integration_steps)
        if L < 0:
            raise ValueError("num_integration_steps must be >= 0")
        return _multinomial_transition(thr, kick_c, drift_c, rng_key, state, logdensity_fn, step_size,
                                       inverse_mass_matrix, L, chain_offset=chain_offset)

    return kernel


def _default_chain_block():
    import os

    v = os.environ.get("BJX_CHAIN_BLOCK", "")
    if v in ("", "auto"):
        return "auto"
    return int(v)  # 0 = all chains in one launch


# MI355X: 256 MiB Infinity Cache in front of HBM.  A chain block whose q, p and g (3 arrays) take
# 192 MiB leaves room for the shared vectors and the callable's scratch.
_IC_WORKING_SET_BYTES = 192 << 20


def auto_chain_block(n_chains: int, dim: int, arrays: int = 3) -> int:
    """Chains per block for ``chain_block="auto"``: the largest multiple of 1024 chains whose
    working set (``arrays`` fp32 arrays per element: q, p, g, plus a per-chain inverse mass matrix
    when there is one) fits the Infinity-Cache budget; all chains at once when the whole batch fits
    or the blocks would be too small to amortise a launch."""
    blk = (_IC_WORKING_SET_BYTES // (4 * int(arrays) * max(int(dim), 1))) // 1024 * 1024
    if blk < 1024 or blk >= n_chains:
        return int(n_chains)
    return int(blk)


class _GraphedTrajectory:
    """HIP-graph capture of the inner loop of one chain block:

        callable(Wq) ; [leapfrog(2 kicks, in place on Wq/Wp) ; callable(Wq)] x (L-1)

    over STATIC workspace buffers (positions ``Wq``, momenta ``Wp``, per-chain step sizes,
    inverse mass matrix), so one captured graph serves every block of every transition: the
    caller fills the workspace (the first kick+drift of a trajectory writes straight into it),
    replays, and reads the end state back.  Removes the per-launch host cost that would
    otherwise dominate once a block is small enough to live in the Infinity Cache.
    """

    def __init__(self, n, D, L, vg, imm_per_chain, device, owner=None):
        self.n, self.D, self.L = n, D, L
        self.owner = owner  # the user's callable: held so that id(owner) in the graph key stays unique
        self.Wq = torch.empty((n, D), dtype=torch.float32, device=device)
        self.Wp = torch.empty((n, D), dtype=torch.float32, device=device)
        self.eps = torch.ones(n, dtype=torch.float32, device=device)
        self.imm = torch.ones((n, D) if imm_per_chain else (D,), dtype=torch.float32, device=device)
        self._lau = Launcher(metrics.Metric("diag", self.imm, D if imm_per_chain else 0, None))
        # the callable's outputs: written in place by callables that can (``_util.eval_into``), so the recording
        # works on q, p and ONE gradient array
        self._g = torch.empty((n, D), dtype=torch.float32, device=device)
        self._logp = torch.empty(n, dtype=torch.float32, device=device)
        self.Wq.zero_()
        self.Wp.zero_()
        self._vg = vg
        # warm-up on a side stream (allocator / lazy-init work must not happen inside capture)
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            self._body()
        torch.cuda.current_stream(device).wait_stream(side)
        torch.cuda.synchronize(device)
        self.graph = new_graph()
        with record_graph(self.graph):
            self.logp, self.g = self._body()

    def _body(self):
        stream = _lib.current_stream()
        # only the last evaluation's logp is read (endpoint proposal): the others are gradient-only where offered
        logp, g = eval_into(self._vg, self.Wq, self._logp, self._g, need_logp=self.L == 1)
        for i in range(self.L - 1):
            self._lau.stage(stream, self.n, self.D, 2, 0.5, 0.5, 1.0, 0.0, self.eps, self.Wq, self.Wp, g, self.Wq,
                            self.Wp)
            # a callable that allocates its own outputs: release the consumed gradient first so the
            # (stream-ordered) allocator hands the same block to it again (working set q, p, g: 3 arrays)
            del logp, g
            logp, g = eval_into(self._vg, self.Wq, self._logp, self._g, need_logp=i == self.L - 2)
        return logp, g


class _GraphCache:
    """The recordings of one kernel (``build_kernel``), keyed on block shape, trajectory length and the USER's
    callable (each recording holds it)."""

    def __init__(self):
        self.graphs: dict = {}
        self.not_capturable: dict = {}  # id -> callable whose capture failed once (the reference keeps the id from
        #                                 being reused by another object)
        self.seen: dict = {}            # calls per key that did not ``force``

    def get(self, n, D, L, vg, fn, imm_per_chain, dev, force):
        """The recording for blocks of ``n`` chains.  ``force`` (``use_graph=True``, and every block of a transition
        that is graphed): record now if there is none, errors propagate.  Otherwise (``use_graph="auto"``): record on
        the SECOND call with a given shape and trajectory length (a one-off call -- or a caller that varies L from
        step to step -- should not pay for a recording), keep at most 8 recordings per kernel, and remember a callable
        that cannot be recorded (or is broken: the plain path re-raises); ``None`` while there is no recording."""
        key = (n, D, L, id(fn), imm_per_chain, dev.index)
        if key in self.graphs:
            return self.graphs[key]
        if not force:
            if id(fn) in self.not_capturable:
                return None
            self.seen[key] = self.seen.get(key, 0) + 1
            if self.seen[key] < 2 or len(self.graphs) >= 8:
                return None
        try:
            self.graphs[key] = _GraphedTrajectory(n, D, L, vg, imm_per_chain, dev, owner=fn)
        except RuntimeError:
            if force:
                raise
            self.not_capturable[id(fn)] = fn
            torch.cuda.synchronize(dev)
            return None
        return self.graphs[key]


_SIDE_STREAMS: dict = {}


def _side_streams(dev, n):
    pool = _SIDE_STREAMS.setdefault(dev.index, [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device=dev))
    return pool[:n]


class _Block(NamedTuple):
    """One chain block of a transition: its rows of the batch arrays, its launcher (per-chain matrices sliced), step
    sizes and chain offset, and its ONE gradient buffer (and logp): its slice of the result arrays, or None when the
    callable's own outputs are adopted."""

    n: int
    sl: slice
    lau: Launcher
    eps_pc: Optional[torch.Tensor]
    off: int
    g_buf: Optional[torch.Tensor]
    logp_buf: Optional[torch.Tensor]


class _Transition:
    """One HMC transition for all chains (hmc.py:279-312 + hmc_proposal.generate 153-176), chain block by chain block.
    The constructor validates the inputs, allocates the result arrays and decides blocking, streams and graphing;
    ``run`` advances the blocks and returns ``(HMCState, HMCInfo)``."""

    def __init__(self, thr, general, kick_c, drift_c, chain_block, streams, use_graph, graphs, rng_key, state,
                 logdensity_fn, step_size, inverse_mass_matrix, num_integration_steps, chain_offset):
        (self.q0, self.logp0, self.g0, N, D, self.key, self.vg, metric, self.eps, self.eps_pc, _,
         self.off) = _prologue(rng_key, state, logdensity_fn, step_size, inverse_mass_matrix, chain_offset)
        q0, logp0 = self.q0, self.logp0
        L = int(num_integration_steps)
        if L < 0:
            raise ValueError("num_integration_steps must be >= 0")
        self.N, self.D, self.L, self.thr = N, D, L, thr
        self.fn, self.graphs, self.dev = logdensity_fn, graphs, q0.device
        self.lau = Launcher(metric, kick_c, drift_c, general)
        graphable = metric.kind == "diag" and not general

        self.p0 = torch.empty_like(q0)
        self.ke0 = torch.empty_like(logp0)
        self.p_end = torch.empty_like(q0)
        self.q_new = torch.empty_like(q0)
        self.g_new = torch.empty_like(q0)
        self.logp_new = torch.empty_like(logp0)
        self.acc_rate = torch.empty_like(logp0)
        self.energy = torch.empty_like(logp0)
        self.is_acc = torch.empty(N, dtype=torch.bool, device=self.dev)
        self.is_div = torch.empty(N, dtype=torch.bool, device=self.dev)

        cb = chain_block
        self.n_streams = 1 if streams == "auto" else streams
        if cb == "auto":  # Infinity-Cache tiling pays for the streaming (diagonal) kernels only
            if metric.kind == "diag":
                cb = auto_chain_block(N, D, 3 + (1 if metric.imm_stride else 0))
            elif metric.kind == "dense" and int(self.n_streams) > 1:
                cb = -(-N // int(self.n_streams) // 128) * 128  # equal blocks of whole 128-row GEMM tiles
            else:
                cb = N
        self.blk = blk = N if not cb or cb >= N else int(cb)
        self.n_blocks = (N + blk - 1) // blk if N else 0
        self.graphed = use_graph is True and L >= 1 and graphable
        if use_graph == "auto" and L >= 2 and N > 0 and graphable and blk * D <= (1 << 21):
            if is_capturable(logdensity_fn):
                self.graphed = graphs.get(min(blk, N), D, L, self.vg, logdensity_fn, metric.imm_stride != 0,
                                          self.dev, force=False) is not None
            else:
                warn_eager_driver(logdensity_fn, "hmc")  # small launches from Python: say so once
        self.single = single = self.n_blocks <= 1 and not self.graphed
        # end-of-trajectory state (HMCInfo.proposal): per-block work buffers are copied out
        # unless the whole batch is one un-graphed block, in which case they ARE the result
        self.q_end = torch.empty_like(q0) if L > 0 else q0
        self.p_work = torch.empty_like(q0) if (L > 0 and not self.graphed) else None
        # (a callable that evaluates into the caller's buffers writes g / logp of every block straight here, one
        # un-graphed block included; the outputs of any other callable are copied in, or adopted when single)
        writes_into = getattr(self.vg, "_bjx_eval_into", None) is not None
        self.g_end = torch.empty_like(q0) if (L > 0 and (not single or writes_into)) else None
        self.logp_end = torch.empty_like(logp0) if (L > 0 and (not single or writes_into)) else None
        if L == 0:
            self.g_end, self.logp_end = self.g0, logp0
        self.fused_first = L > 0 and not self.graphed and self.lau.fuses_first(D)

    def _block(self, b):
        s, e = b * self.blk, min(self.N, (b + 1) * self.blk)
        sl = slice(s, e)
        g_buf = logp_buf = None
        if self.L > 0 and self.g_end is not None:
            g_buf, logp_buf = (self.g_end, self.logp_end) if self.single else (self.g_end[sl], self.logp_end[sl])
        return _Block(e - s, sl, self.lau.rows(sl), None if self.eps_pc is None else self.eps_pc[sl], self.off + s,
                      g_buf, logp_buf)

    def _evaluate(self, blk, q, need_logp):
        """One log-density evaluation of the trajectory; ``need_logp`` is true for the last one only."""
        if blk.g_buf is None:
            return eval_logdensity(self.vg, q)
        return eval_into(self.vg, q, blk.logp_buf, blk.g_buf, need_logp)

    def _stepwise(self, blk):
        """The trajectory as plain launches, one per position update (generalized_two_stage_integrator,
        integrators.py:104-150: the closing kick b_K of a step merges with the opening kick b_1 of the next; velocity
        Verlet is the one-stage case, its first update possibly done by the momentum launch).  A generator: yields
        after every log-density evaluation so that several blocks can be advanced in turn on their own streams."""
        stream = _lib.current_stream()
        sl, stage, n, D, eps, eps_pc = blk.sl, blk.lau.stage, blk.n, self.D, self.eps, blk.eps_pc
        last = (self.L - 1, len(blk.lau.drift_c) - 1)
        q_in, p_in, g = self.q0[sl], self.p0[sl], self.g0[sl]
        q, p = self.q_end[sl], self.p_work[sl]
        logp = None
        for i, si, n_kicks, ka, kb, a in blk.lau.updates(self.L):
            if q_in is q or not self.fused_first:  # (the momentum launch has done the first update)
                p = stage(stream, n, D, n_kicks, ka, kb, a, eps, eps_pc, q_in, p_in, g, q, p)
            q_in, p_in = q, p
            # consumed: a callable that allocates its own outputs gets the same block back from the
            # (stream-ordered) allocator, so the block's working set stays q, p, g (3 arrays)
            del logp, g
            logp, g = self._evaluate(blk, q, (i, si) == last)
            yield
            stream = _lib.current_stream()
        return q, p, logp, g

    def _graphed(self, blk):
        """The trajectory as one graph replay: the first kick + drift writes straight into the static workspace."""
        sl, m = blk.sl, blk.lau.metric
        ctx = self.graphs.get(blk.n, self.D, self.L, self.vg, self.fn, m.imm_stride != 0, self.dev, force=True)
        if blk.eps_pc is None:
            ctx.eps.fill_(self.eps)
        else:
            ctx.eps.copy_(blk.eps_pc)
        ctx.imm.copy_(m.imm)
        blk.lau.stage(_lib.current_stream(), blk.n, self.D, 1, 0.5, 0.0, 1.0, self.eps, blk.eps_pc, self.q0[sl],
                      self.p0[sl], self.g0[sl], ctx.Wq, ctx.Wp)
        ctx.graph.replay()
        return ctx.Wq, ctx.Wp, ctx.logp, ctx.g

    def _finish(self, blk, eps, eps_pc, q, p, logp, g):
        """Closing kick + accept / reject of one block, and its end state into the result arrays."""
        sl = blk.sl
        blk.lau.finish(_lib.current_stream(), self.key, blk.off, blk.n, self.D, eps, eps_pc, self.thr, self.q0[sl],
                       self.logp0[sl], self.g0[sl], self.ke0[sl], q, logp, g, p, self.p_end[sl], self.q_new[sl],
                       self.logp_new[sl], self.g_new[sl], self.acc_rate[sl], self.is_acc[sl], self.is_div[sl],
                       self.energy[sl])
        if self.L > 0:
            if g is blk.g_buf:  # (and logp is logp_buf: the last evaluation is never gradient-only)
                pass            # the callable wrote the block's end state where it belongs
            elif self.single:
                self.g_end, self.logp_end = g, logp
            else:
                self.g_end[sl].copy_(g)
                self.logp_end[sl].copy_(logp)
            if self.graphed:
                self.q_end[sl].copy_(q)

    def run_block(self, b):
        """One chain block's transition as a generator (see ``_stepwise``)."""
        blk = self._block(b)
        sl = blk.sl
        stream = _lib.current_stream()
        if self.fused_first:
            blk.lau.momentum_kick(stream, self.key, blk.off, blk.n, self.D, self.eps, blk.eps_pc, self.q0[sl],
                                  self.g0[sl], self.p0[sl], self.ke0[sl], self.q_end[sl], self.p_work[sl])
        else:
            blk.lau.momentum(stream, self.key, blk.off, blk.n, self.D, self.p0[sl], self.ke0[sl])
        if self.L == 0:
            self._finish(blk, 0.0, None, self.q0[sl], self.p0[sl], self.logp0[sl], self.g0[sl])
        elif self.graphed:
            self._finish(blk, self.eps, blk.eps_pc, *self._graphed(blk))
        else:
            self._finish(blk, self.eps, blk.eps_pc, *(yield from self._stepwise(blk)))

    def run(self):
        """Blocks are independent, so up to ``streams`` of them are advanced in turn, each on its own HIP stream: one
        block's callable (bandwidth-bound), the start-up of its launches and the output drain of a dense-metric GEMM
        then overlap another block's kernels."""
        n_blocks = self.n_blocks
        ns = 1 if (self.graphed or n_blocks <= 1) else min(int(self.n_streams), n_blocks)
        if ns <= 1:
            for b in range(n_blocks):
                for _ in self.run_block(b):
                    pass
        else:
            main = torch.cuda.current_stream(self.dev)
            pool = _side_streams(self.dev, ns)
            for st_ in pool:
                st_.wait_stream(main)
            for w0 in range(0, n_blocks, ns):
                active = [(self.run_block(b), pool[b - w0]) for b in range(w0, min(w0 + ns, n_blocks))]
                while active:
                    for item in list(active):
                        with torch.cuda.stream(item[1]):
                            try:
                                next(item[0])
                            except StopIteration:
                                active.remove(item)
            for st_ in pool:
                main.wait_stream(st_)
        if n_blocks == 0 and self.L > 0:
            self.g_end, self.logp_end = self.g0, self.logp0
        info = HMCInfo(self.p0, self.acc_rate, self.is_acc, self.is_div, self.energy,
                       IntegratorState(self.q_end, self.p_end, self.logp_end, self.g_end), self.L)
        return HMCState(self.q_new, self.logp_new, self.g_new), info


def build_kernel(integrator=integrators.velocity_verlet, divergence_threshold: float = 1000,
                 build_proposal=None, *, chain_block=None, use_graph="auto", streams="auto"):
    """blackjax/mcmc/hmc.py:251-314.  ``build_proposal`` other than the default endpoint
    proposal (hmc_proposal, 115-178) is out of scope.

    ``chain_block``: chains are independent, so a transition may be run block by block
    (``chain_block`` chains at a time through all L leapfrogs) instead of launch by launch
    over all N chains.  With a block whose q/p/g working set fits the 256 MiB Infinity Cache
    the L-step loop re-reads its state from on-die cache instead of HBM.  Results are
    identical for any blocking (per-chain keys depend only on the global chain index).
    ``chain_block="auto"`` sizes the block for the 256 MiB Infinity Cache (``auto_chain_block``);
    measured at 65 536 x 1 024, L = 50: +12 % whole-transition throughput over one block.

    ``streams``: chain blocks advanced concurrently, each on its own HIP stream (blocks are
    independent; results are identical for any value), so that one block's callable and launch
    ramps overlap another block's kernels.  Measured: 65 536 x 1 024 diagonal, two blocks of 8 192
    in flight 234.5 vs 228.0 M/s with one stream (+2.9 %; the host then issues launches for two
    queues); 16 384 x 512 dense, two half batches: the GEMM launches shorten from 91 to 83 us each
    but the transition does not (2.46 vs 2.42 ms).  ``"auto"`` = 1.

    ``use_graph``: capture the per-block inner loop (the user's callable included) in a HIP
    graph (diagonal metric; the callable must be capturable: static shapes, no host sync).
    ``"auto"`` (default): do so for callables DECLARED recordable (``blackjax_amd.targets``, or any
    callable passed through ``blackjax_amd.capturable``) when a block is small enough for its
    launches to be bound by the host's launch rate (at most 2^21 elements: a leapfrog launch is
    then under ~10 us of GPU work; at 65 536 x 1 024 graphs measured no faster than plain
    launches), with a fall-back to plain launches if the recording fails; every other callable
    is driven with plain launches.  ``True`` records whatever the callable is.  As under
    ``jax.jit`` in the reference, a recorded callable is replayed as recorded: Python-side state
    it reads (a minibatch index, say) is frozen at recording time.
    """
    if use_graph not in (True, False, "auto"):
        raise ValueError("use_graph must be True, False or 'auto'")
    thr = float(divergence_threshold)
    # any palindromic coefficient list [b1, a1, ..., b1] (integrators.py:62-152); the higher-order
    # ones (mclachlan / yoshida / omelyan) run through the general-coefficient kernels
    integrators.check_supported(integrator, allow_general=True)
    kick_c = integrator.coefficients[0::2]   # b1 .. b1
    drift_c = integrator.coefficients[1::2]  # a1 ..
    if build_proposal is multinomial_hmc_proposal:
        return _build_mhmc_kernel(thr, kick_c, drift_c)
    if build_proposal not in (None, hmc_proposal):
        raise NotImplementedError(
            "build_proposal must be hmc_proposal (default) or multinomial_hmc_proposal")
    general = integrator is not integrators.velocity_verlet
    if chain_block is None:
        chain_block = _default_chain_block()
    graphs = _GraphCache()

    def kernel(rng_key, state: HMCState, logdensity_fn: Callable, step_size,
               inverse_mass_matrix, num_integration_steps: int, *, chain_offset: int = 0):
        return _Transition(thr, general, kick_c, drift_c, chain_block, streams, use_graph, graphs, rng_key, state,
                           logdensity_fn, step_size, inverse_mass_matrix, num_integration_steps, chain_offset).run()

    return kernel


def build_fused_target_kernel(divergence_threshold: float = 1000, *, with_info_arrays: bool = True):
    """A whole transition per launch for log-densities the ENGINE evaluates itself (``bjx_hmc_trajectory_diag``):
    ``blackjax_amd.targets.NealFunnel`` / ``DiagGaussian``, diagonal metric, velocity Verlet, 128 < D <= 1 024,
    D % 4 == 0.  OUTSIDE the external-callable contract (the reference calls ``logdensity_fn`` between two
    leapfrogs) -- opt-in through ``hmc(..., fuse_target=True)``; state and info are bit for bit those of
    ``build_kernel()``'s kernel.  ``with_info_arrays=False``: ``HMCInfo.momentum`` and ``.proposal`` are ``None``
    and their five arrays are not written."""
    thr = float(divergence_threshold)

    def kernel(rng_key, state: HMCState, logdensity_fn: Callable, step_size,
               inverse_mass_matrix, num_integration_steps: int, *, chain_offset: int = 0):
        q0, logp0, g0, N, D, (k0, k1, fold), _, metric, eps, eps_pc, _, _ = _prologue(
            rng_key, state, logdensity_fn, step_size, inverse_mass_matrix, chain_offset)
        dev = q0.device
        L = int(num_integration_steps)
        spec = getattr(logdensity_fn, "_bjx_fused_target", None)
        spec = spec(D) if callable(spec) else None
        if spec is None or metric.kind != "diag" or D % 4 != 0 or not 128 < D <= 1024 or L < 1:
            raise NotImplementedError(
                "fuse_target=True needs a blackjax_amd.targets log-density the engine can evaluate in place "
                "(NealFunnel; DiagGaussian), a diagonal metric, 128 < D <= 1024 with D % 4 == 0 and at least "
                "one integration step")
        q_new, g_new, logp_new = torch.empty_like(q0), torch.empty_like(g0), torch.empty_like(logp0)
        acc_rate, energy = torch.empty_like(logp0), torch.empty_like(logp0)
        is_acc = torch.empty(N, dtype=torch.bool, device=dev)
        is_div = torch.empty(N, dtype=torch.bool, device=dev)
        p0 = q1 = p_end = logp1 = g1 = None
        if with_info_arrays:
            p0, q1, p_end, g1 = (torch.empty_like(q0) for _ in range(4))
            logp1 = torch.empty_like(logp0)
        if spec[0] == "rtc":
            # a user-written device target (targets.DeviceTarget): the same trajectory code, compiled around it
            # by hiprtc (csrc/bjx_traj_dev.h, blackjax_amd/rtc.py)
            from . import rtc

            tgt = spec[1]
            ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
            args = rtc.TrajArgs(k0, k1, int(chain_offset), fold, N, D, L, eps, ptr(eps_pc), metric.imm.data_ptr(),
                                metric.imm_stride, thr, tgt._params_ptr(dev), q0.data_ptr(), logp0.data_ptr(),
                                g0.data_ptr(), ptr(p0), ptr(q1), ptr(p_end), ptr(logp1), ptr(g1), q_new.data_ptr(),
                                logp_new.data_ptr(), g_new.data_ptr(), acc_rate.data_ptr(), energy.data_ptr(),
                                is_acc.data_ptr(), is_div.data_ptr())
            tgt.module().launch(f"bjx_rtc_traj_{rtc.ni_for(D)}", min((N + 3) // 4, 65536), 256,
                                _lib.current_stream(), args)
        else:
            _lib.call("bjx_hmc_trajectory_diag", _lib.current_stream(), k0, k1, int(chain_offset), fold, N, D, L,
                      eps, _lib.ptr(eps_pc), metric.imm.data_ptr(), metric.imm_stride, thr, int(spec[0]),
                      _lib.ptr(spec[1]), q0.data_ptr(), logp0.data_ptr(), g0.data_ptr(), _lib.ptr(p0),
                      _lib.ptr(q1), _lib.ptr(p_end), _lib.ptr(logp1), _lib.ptr(g1), q_new.data_ptr(),
                      logp_new.data_ptr(), g_new.data_ptr(), acc_rate.data_ptr(), is_acc.data_ptr(),
                      is_div.data_ptr(), energy.data_ptr())
        proposal = IntegratorState(q1, p_end, logp1, g1) if with_info_arrays else None
        return HMCState(q_new, logp_new, g_new), HMCInfo(p0, acc_rate, is_acc, is_div, energy, proposal, L)

    return kernel


def as_top_level_api(logdensity_fn: Callable, step_size, inverse_mass_matrix,
                     num_integration_steps: int, *, divergence_threshold: float = 1000,
                     integrator=integrators.velocity_verlet, build_proposal=None,
                     chain_offset: int = 0, chain_block=None,
                     use_graph="auto", streams="auto", fuse_target=False) -> SamplingAlgorithm:
    """blackjax/mcmc/hmc.py:317-414.  ``chain_offset`` is this process' first global chain
    index when the chains of one run are sharded over several GPUs.  ``fuse_target=True`` (or ``"lean"``: without
    the momentum / proposal arrays of ``HMCInfo``): ``build_fused_target_kernel`` -- one launch per transition for
    the library's own log-densities, outside the external-callable contract, identical results."""
    if fuse_target:
        if integrator is not integrators.velocity_verlet or build_proposal not in (None, hmc_proposal):
            raise NotImplementedError("fuse_target=True: velocity Verlet with the endpoint proposal")
        kernel = build_fused_target_kernel(divergence_threshold, with_info_arrays=fuse_target != "lean")
    else:
        kernel = build_kernel(integrator, divergence_threshold, build_proposal,
                              chain_block=chain_block, use_graph=use_graph, streams=streams)

    def init_fn(position, rng_key=None):
        del rng_key
        return init(position, logdensity_fn)

    def step_fn(rng_key, state):
        return kernel(rng_key, state, logdensity_fn, step_size, inverse_mass_matrix,
                      num_integration_steps, chain_offset=chain_offset)

    return SamplingAlgorithm(init_fn, step_fn)
