"""What ``meanfield_vi`` and ``fullrank_vi`` share: the argument checks, the call of a family's reduction and the
bodies of ``step`` and ``as_top_level_api``.  A family is a Gaussian ``q`` with a ``(D,)`` mean ``mu`` and a second
parameter vector (``rho``, ``chol_params``); it passes in its name, C symbol, checker, ``_draw`` and tuples."""
from __future__ import annotations

from typing import Callable

import torch

from .. import _lib
from .._util import check_batch, eval_into, value_and_grad
from ..base import VIAlgorithm
from ..random import key_words


def num_samples(num_samples) -> int:
    s = int(num_samples)
    if s < 1:
        raise ValueError(f"num_samples must be at least 1, got {num_samples}")
    return s


def position(position) -> torch.Tensor:
    """The ``(dim,)`` tensor ``init`` takes shape and device from."""
    position = check_batch(position, "position")
    if position.ndim != 1 or position.shape[0] < 1:
        raise ValueError(f"position must be (dim,), got {tuple(position.shape)}")
    return position


def kl_and_grad(name: str, symbol: str, parameters: Callable, rng_key, mu, second, logp, grad, stl_estimator: bool):
    """-> ``(kl, g_mu, g_second)`` from the reduction ``symbol`` (its workspace query is ``symbol_workspace_bytes``)
    of the family ``name``, whose ``parameters(mu, second, what)`` checks the pair."""
    mu, second = parameters(mu, second, "parameters")
    logp, G = check_batch(logp, "logp"), check_batch(grad, "grad")
    D = mu.shape[0]
    if G.ndim != 2 or G.shape[1] != D or G.shape[0] < 1 or logp.shape != G.shape[:1]:
        raise ValueError(f"logp and grad must be (num_samples,) and (num_samples, {D}), got {tuple(logp.shape)} and "
                         f"{tuple(G.shape)}")
    if logp.device != mu.device or G.device != mu.device:
        raise ValueError(f"logp and grad must be on {mu.device}, got {logp.device} and {G.device}")
    S = G.shape[0]
    k0, k1 = key_words(rng_key)
    nbytes = getattr(_lib.load(), symbol + "_workspace_bytes")(S, D)
    if nbytes <= 0:
        raise ValueError(f"{name}: {S} draws of dimension {D} are out of range (include/bjx_hip.h, VI)")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=mu.device)
    g_mu, g_second = torch.empty_like(mu), torch.empty_like(second)
    kl = torch.empty((), dtype=torch.float32, device=mu.device)
    with torch.cuda.device(mu.device):
        _lib.call(symbol, _lib.current_stream(), k0, k1, S, D, 1 if stl_estimator else 0, G.data_ptr(),
                  logp.data_ptr(), second.data_ptr(), ws.data_ptr(), g_mu.data_ptr(), g_second.data_ptr(),
                  kl.data_ptr())
    return kl, g_mu, g_second


def step(draw: Callable, kl_and_grad: Callable, State, Info, rng_key, mu, second, opt_state, logdensity_fn: Callable,
         optimizer, num_samples_, stl_estimator: bool):
    """One stochastic gradient step on the KL estimate from a family's checked parameters, with its ``_draw`` and
    ``kl_and_grad`` -> ``(State, Info)``."""
    S = num_samples(num_samples_)
    k0, k1 = key_words(rng_key)
    vg = value_and_grad(logdensity_fn)
    with torch.cuda.device(mu.device):
        z = draw(k0, k1, mu, second, S)
        logp, G = eval_into(vg, z, torch.empty(S, dtype=torch.float32, device=mu.device), torch.empty_like(z))
        kl, g_mu, g_second = kl_and_grad((k0, k1), mu, second, logp, G, stl_estimator)
        updates, opt_state = optimizer.update((g_mu, g_second), opt_state, (mu, second))
        u_mu, u_second = updates
        return State(mu + u_mu, second + u_second, opt_state), Info(kl)


def as_top_level_api(init: Callable, step: Callable, sample: Callable, logdensity_fn: Callable, optimizer,
                     num_samples: int) -> VIAlgorithm:
    def init_fn(position):
        return init(position, optimizer)

    def step_fn(rng_key, state):
        return step(rng_key, state, logdensity_fn, optimizer, num_samples)

    def sample_fn(rng_key, state, num_samples: int = 1):
        return sample(rng_key, state, num_samples)

    return VIAlgorithm(init_fn, step_fn, sample_fn)
