"""Batched independent Rosenbluth-Metropolis-Hastings on MI355X behind the ``blackjax.irmh`` API surface.

Mirrors blackjax/mcmc/irmh.py: ``init``, ``build_kernel`` and ``as_top_level_api``; state, info and the accept are those
of blackjax/mcmc/random_walk.py (``RWState``, ``RWInfo``, ``build_rmh``).  The proposal does not depend on the current
position: ``proposal_distribution(rng_key) -> (N, D)`` is batched and receives the transition's ``rng_key`` unchanged
(the reference hands it ``key_proposal``; ``blackjax_amd.random.chain_normal(..., child=0)`` draws from that key).

``proposal_logdensity_fn(a, b)`` is the log-density of proposing ``b`` FROM ``a`` (both ``RWState``); for an
independent proposal of density ``q`` that is ``log q(b.position)``.  It is called with ``(initial, proposed)`` and
with ``(proposed, initial)``; without it the proposal is taken to be symmetric.  See ``blackjax_amd.random_walk``.
"""
from __future__ import annotations

from typing import Callable

from . import random_walk
from .base import SamplingAlgorithm
from .random_walk import RWInfo, RWState

__all__ = ["RWState", "RWInfo", "init", "build_kernel", "as_top_level_api"]

init = random_walk.init


def build_kernel():
    """blackjax/mcmc/irmh.py ``build_kernel``."""

    def kernel(rng_key, state: RWState, logdensity_fn: Callable, proposal_distribution: Callable,
               proposal_logdensity_fn=None, *, chain_offset: int = 0):
        q0, logp0 = random_walk._check_state(state)
        q1 = random_walk._check_generated(proposal_distribution(rng_key), q0, "proposal_distribution's draw")
        return random_walk._finish(rng_key, int(chain_offset), q0, logp0, q1, logdensity_fn, proposal_logdensity_fn)

    return kernel


def as_top_level_api(logdensity_fn: Callable, proposal_distribution: Callable, proposal_logdensity_fn=None, *,
                     chain_offset: int = 0) -> SamplingAlgorithm:
    """blackjax/mcmc/irmh.py ``as_top_level_api``: ``init(position)``, ``step(rng_key, state)``."""
    kernel = build_kernel()

    def init_fn(position, rng_key=None):
        del rng_key
        return init(position, logdensity_fn)

    def step_fn(rng_key, state):
        return kernel(rng_key, state, logdensity_fn, proposal_distribution, proposal_logdensity_fn,
                      chain_offset=chain_offset)

    return SamplingAlgorithm(init_fn, step_fn)
