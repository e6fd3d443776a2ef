"""Batched random-walk Metropolis on MI355X behind the ``blackjax.rmh`` / ``blackjax.additive_step_random_walk`` API
surface.

Mirrors blackjax/mcmc/random_walk.py: ``RWState``, ``RWInfo``, ``init``, ``normal``, ``build_additive_step``,
``build_rmh`` (``transition_energy``, ``kernel``, ``rmh_proposal``), ``additive_step_random_walk`` with its
``normal_random_walk`` factory, and ``rmh_as_top_level_api``; the accept is
mcmc/proposal.py::compute_asymmetric_acceptance_ratio + ``static_binomial_sampling`` on ``safe_energy_diff``.  No
gradient is ever taken: the log-density is evaluated VALUE ONLY (``_util.eval_value``), so a callable that cannot be
differentiated works, and inside tempered SMC a move costs no autograd pass.  There is no warm-up, as in the reference.

The chain axis is native; chain ``i`` of ``step(rng_key, state)`` reproduces the reference's single-chain
``step(jax.random.split(rng_key, N)[chain_offset + i], state_i)``.  Like every RNG-dependent part of the package,
parity with a real JAX run is unpinned; the arithmetic is held against a NumPy restatement of the
reference (tests/random_walk_restatement.py).

Differences from the reference, all deliberate:

* User-written generators are batched -- ``transition_generator(rng_key, position (N, D)) -> (N, D)`` -- and receive
  the transition's ``rng_key`` UNCHANGED (a plain key or a ``ChainMajorKey``), where the reference hands them
  ``key_proposal``.  ``blackjax_amd.random.chain_normal(rng_key, N, D, device=..., child=0)`` draws from exactly that
  ``key_proposal`` of every chain; ``chain_offset`` is the generator's own business.
* ``normal(sigma)`` returns an object the kernel recognises and runs fused on the device (one launch: keyed normal
  plus scaled add).  ``sigma`` is shared by all chains: a scalar, ``(D,)`` (one scale per dimension) or ``(D, D)`` -- a
  2-d ``sigma`` is always a matrix applied as ``sigma @ z``, so there is no ``N == D`` ambiguity.  Per-chain sigmas are
  not supported.
* ``proposal_logdensity_fn(a, b)`` is the log-density of proposing ``b`` FROM ``a`` (both ``RWState``), returning
  ``(N,)``.  It is called twice per transition: with ``(initial, proposed)`` and with ``(proposed, initial)``.

The arithmetic runs in libbjxhip (include/bjx_hip.h, "random walk"); this module sequences
propose (one launch; a dense ``sigma`` adds a noise launch and the MFMA GEMM) -> user callable -> finish (one launch).
"""
from __future__ import annotations

from typing import Callable, NamedTuple

import torch

from . import _lib
from ._util import check_batch, eval_value
from .base import SamplingAlgorithm
from .random import key_spec

__all__ = ["RWState", "RWInfo", "init", "normal", "build_additive_step", "build_rmh", "additive_step_random_walk",
           "normal_random_walk", "rmh_as_top_level_api"]


class RWState(NamedTuple):
    """blackjax/mcmc/random_walk.py ``RWState``, batched: (N, D), (N,)."""

    position: torch.Tensor
    logdensity: torch.Tensor


class RWInfo(NamedTuple):
    """blackjax/mcmc/random_walk.py ``RWInfo``, batched: (N,) float32, (N,) bool, and the proposed state -- the very
    tensors the transition produced, not copies."""

    acceptance_rate: torch.Tensor
    is_accepted: torch.Tensor
    proposal: RWState


def init(position: torch.Tensor, logdensity_fn: Callable) -> RWState:
    """blackjax/mcmc/random_walk.py ``init``: the log-density (value only) at the initial positions."""
    position = check_batch(position, "position")
    if position.ndim != 2:
        raise ValueError(f"position must be (n_chains, dim), got {tuple(position.shape)}")
    return RWState(position, eval_value(logdensity_fn, position))


class _NormalStep:
    """The callable ``normal(sigma)`` returns.  Called directly, ``random_step(rng_key, position)`` gives the move
    ``sigma * z`` (``sigma @ z`` when dense) with ``z_i = normal(key_proposal of chain i, (D,))`` -- the move the kernel
    makes from the same ``rng_key``; the kernel itself fuses the draw, the scale and the add into one launch."""

    def __init__(self, sigma):
        s = sigma if isinstance(sigma, torch.Tensor) else torch.as_tensor(sigma)
        if s.ndim > 2:
            raise ValueError(f"The scale has the wrong number of dimensions: expected 0, 1 or 2, got {s.ndim}.")
        if s.ndim == 2 and s.shape[0] != s.shape[1]:
            raise ValueError(f"a 2-d sigma is a dense matrix and must be square, got {tuple(s.shape)} "
                             "(per-chain sigmas are not supported)")
        self.sigma = s
        self.ndim = s.ndim
        self._scalar = float(s) if s.ndim == 0 else 0.0  # (a 0-d device tensor is read once, here)
        self._prepared: dict = {}  # (D, device) -> (D,) scales, or sigma^T (D, D) row-major

    def _check(self, N: int, D: int) -> None:
        """Shape of ``sigma`` against the batch (host-side: no device is touched)."""
        s = self.sigma
        if s.ndim == 1 and s.shape[0] != D:
            if s.shape[0] == N:
                raise NotImplementedError(f"a per-chain sigma is not supported: a 1-d sigma holds one scale per "
                                          f"dimension ({D}), got {s.shape[0]} entries")
            raise ValueError(f"sigma has {s.shape[0]} entries, position has {D} dims")
        if s.ndim == 2 and s.shape[0] != D:
            raise ValueError(f"sigma is {tuple(s.shape)}, position has {D} dims")

    def _device_sigma(self, D: int, device):
        t = self._prepared.get((D, device))
        if t is None:
            t = self.sigma.detach().to(device=device, dtype=torch.float32)
            t = (t.t() if t.ndim == 2 else t).contiguous()  # noise @ sigma^T: row i = sigma @ z_i
            self._prepared[(D, device)] = t
        return t

    def _propose(self, k0, k1, fold, off, q0: torch.Tensor) -> torch.Tensor:
        """q0 + move, out of place."""
        N, D = q0.shape
        self._check(N, D)
        stream = _lib.current_stream()
        q1 = torch.empty_like(q0)
        diag = lin = None
        if self.ndim == 1:
            diag = self._device_sigma(D, q0.device)
        elif self.ndim == 2 and N > 0:
            noise, lin = torch.empty_like(q0), torch.empty_like(q0)
            _lib.call("bjx_rw_noise", stream, k0, k1, off, fold, 0, N, D, noise.data_ptr())
            _lib.call("bjx_dense_matmul", stream, N, D, noise.data_ptr(), self._device_sigma(D, q0.device).data_ptr(),
                      lin.data_ptr())
        _lib.call("bjx_rw_propose", stream, k0, k1, off, fold, N, D, self._scalar, _lib.ptr(diag), _lib.ptr(lin),
                  q0.data_ptr(), q1.data_ptr())
        return q1

    def __call__(self, rng_key, position: torch.Tensor, *, chain_offset: int = 0) -> torch.Tensor:
        position = check_batch(position, "position")
        if position.ndim != 2:
            raise ValueError(f"position must be (n_chains, dim), got {tuple(position.shape)}")
        k0, k1, fold = key_spec(rng_key)
        return self._propose(k0, k1, fold, int(chain_offset), torch.zeros_like(position))  # fma(s, z, 0) = s * z


def normal(sigma) -> Callable:
    """blackjax/mcmc/random_walk.py ``normal``: the Gaussian random step ``random_step(rng_key, position) -> move``.
    ``sigma``: a Python or 0-d scalar, ``(D,)`` (one scale per dimension) or ``(D, D)`` (applied as ``sigma @ z``),
    shared by all chains.  More than two dimensions, or a 2-d ``sigma`` that is not square, raise ``ValueError``; a 1-d
    ``sigma`` with one entry per chain raises ``NotImplementedError`` at the first transition."""
    return _NormalStep(sigma)


def _check_state(state) -> tuple:
    q0 = check_batch(state.position, "state.position")
    logp0 = check_batch(state.logdensity, "state.logdensity")
    if q0.ndim != 2:
        raise ValueError(f"state.position must be (n_chains, dim), got {tuple(q0.shape)}")
    if logp0.shape != q0.shape[:1]:
        raise ValueError(f"state.logdensity must be ({q0.shape[0]},), got {tuple(logp0.shape)}")
    return q0, logp0


def _check_generated(x, q0: torch.Tensor, what: str) -> torch.Tensor:
    x = check_batch(x, what)
    if x.shape != q0.shape:
        raise ValueError(f"{what} must be {tuple(q0.shape)}, got {tuple(x.shape)}")
    return x


def _finish(rng_key, chain_offset: int, q0, logp0, q1, logdensity_fn: Callable, proposal_logdensity_fn=None):
    """The second half of every transition of the family: the log-density at the proposal (value only), the two
    proposal log-densities of an asymmetric proposal, then accept and select in one launch (``bjx_rw_finish``)."""
    N, D = q0.shape
    k0, k1, fold = key_spec(rng_key)
    logp1 = eval_value(logdensity_fn, q1)
    initial, proposed = RWState(q0, logp0), RWState(q1, logp1)
    f_ip = f_pi = None
    if proposal_logdensity_fn is not None:
        f_ip = _check_proposal_logdensity(proposal_logdensity_fn(initial, proposed), N)  # of proposing q1 from q0
        f_pi = _check_proposal_logdensity(proposal_logdensity_fn(proposed, initial), N)  # of proposing q0 from q1
    q_new, logp_new, acc_rate = torch.empty_like(q0), torch.empty_like(logp0), torch.empty_like(logp0)
    is_acc = torch.empty(N, dtype=torch.bool, device=q0.device)  # one byte per flag, 0 / 1: written as uint8
    _lib.call("bjx_rw_finish", _lib.current_stream(), k0, k1, int(chain_offset), fold, N, D, q0.data_ptr(),
              logp0.data_ptr(), q1.data_ptr(), logp1.data_ptr(), _lib.ptr(f_ip), _lib.ptr(f_pi), q_new.data_ptr(),
              logp_new.data_ptr(), acc_rate.data_ptr(), is_acc.data_ptr())
    return RWState(q_new, logp_new), RWInfo(acc_rate, is_acc, proposed)


def _check_proposal_logdensity(f, N: int) -> torch.Tensor:
    f = check_batch(f.detach() if isinstance(f, torch.Tensor) else f, "proposal_logdensity_fn's value")
    if f.shape != (N,):
        raise ValueError(f"proposal_logdensity_fn must return shape ({N},), got {tuple(f.shape)}")
    return f


def build_additive_step():
    """blackjax/mcmc/random_walk.py ``build_additive_step``: the proposal is ``position + random_step(key, position)``
    and is symmetric.  ``random_step`` is ``normal(sigma)`` (fused on the device) or any batched callable
    ``(rng_key, position (N, D)) -> move (N, D)``, which receives ``rng_key`` unchanged."""

    def kernel(rng_key, state: RWState, logdensity_fn: Callable, random_step: Callable, *, chain_offset: int = 0):
        q0, logp0 = _check_state(state)
        N, D = q0.shape
        off = int(chain_offset)
        k0, k1, fold = key_spec(rng_key)
        if isinstance(random_step, _NormalStep):
            q1 = random_step._propose(k0, k1, fold, off, q0)
        else:
            move = _check_generated(random_step(rng_key, q0), q0, "random_step's move")
            q1 = torch.empty_like(q0)
            _lib.call("bjx_rw_propose", _lib.current_stream(), k0, k1, off, fold, N, D, 0.0, None, move.data_ptr(),
                      q0.data_ptr(), q1.data_ptr())
        return _finish(rng_key, off, q0, logp0, q1, logdensity_fn)

    return kernel


def build_rmh():
    """blackjax/mcmc/random_walk.py ``build_rmh``: ``transition_generator(rng_key, position (N, D)) -> (N, D)`` proposes;
    without ``proposal_logdensity_fn`` the proposal is taken to be symmetric."""

    def kernel(rng_key, state: RWState, logdensity_fn: Callable, transition_generator: Callable,
               proposal_logdensity_fn=None, *, chain_offset: int = 0):
        q0, logp0 = _check_state(state)
        q1 = _check_generated(transition_generator(rng_key, q0), q0, "transition_generator's proposal")
        return _finish(rng_key, int(chain_offset), q0, logp0, q1, logdensity_fn, proposal_logdensity_fn)

    return kernel


def additive_step_random_walk(logdensity_fn: Callable, random_step: Callable, *,
                              chain_offset: int = 0) -> SamplingAlgorithm:
    """blackjax/mcmc/random_walk.py ``additive_step_random_walk``: ``init(position)``, ``step(rng_key, state)``."""
    kernel = build_additive_step()

    def init_fn(position, rng_key=None):
        del rng_key
        return init(position, logdensity_fn)

    def step_fn(rng_key, state):
        return kernel(rng_key, state, logdensity_fn, random_step, chain_offset=chain_offset)

    return SamplingAlgorithm(init_fn, step_fn)


def normal_random_walk(logdensity_fn: Callable, sigma, *, chain_offset: int = 0) -> SamplingAlgorithm:
    """blackjax/mcmc/random_walk.py ``normal_random_walk``: ``additive_step_random_walk`` with ``normal(sigma)``."""
    return additive_step_random_walk(logdensity_fn, normal(sigma), chain_offset=chain_offset)


def rmh_as_top_level_api(logdensity_fn: Callable, proposal_generator: Callable, proposal_logdensity_fn=None, *,
                         chain_offset: int = 0) -> SamplingAlgorithm:
    """blackjax/mcmc/random_walk.py ``rmh_as_top_level_api``: ``init(position)``, ``step(rng_key, state)``."""
    kernel = build_rmh()

    def init_fn(position, rng_key=None):
        del rng_key
        return init(position, logdensity_fn)

    def step_fn(rng_key, state):
        return kernel(rng_key, state, logdensity_fn, proposal_generator, proposal_logdensity_fn,
                      chain_offset=chain_offset)

    return SamplingAlgorithm(init_fn, step_fn)
