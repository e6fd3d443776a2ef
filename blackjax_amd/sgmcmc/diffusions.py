"""One step of the stochastic-gradient diffusions on MI355X, behind ``blackjax.sgmcmc.diffusions``.

Mirrors blackjax/sgmcmc/diffusions.py: ``overdamped_langevin``, ``sghmc`` and ``sgnht``, each returning a ``one_step``
over the whole ``(N, D)`` chain batch.  A step is one launch of libbjxhip (include/bjx_hip.h, "SGMCMC") that reads the
position (and momentum) and the gradient estimate, draws its normals in registers and writes the new state out of
place; there is no noise tensor.

``rng_key`` is the key of the TRANSITION: chain ``i`` uses ``kc = split(rng_key, .)[chain_offset + i]`` (a
``ChainMajorKey``: its step-fold child).  ``step_size`` and ``temperature`` are each a Python float or a per-chain
``(N,)`` device tensor; they are kernel arguments and compile nothing.  Nothing tests for non-finite values: a NaN
gradient gives a NaN row, as in the reference.
"""
from __future__ import annotations

import torch

from .. import _lib
from .._util import check_batch, step_size_args
from ..random import key_spec

__all__ = ["overdamped_langevin", "sghmc", "sgnht"]


def _per_chain(value, n_chains: int, device, name: str):
    """``step_size_args`` for the argument called ``name``."""
    try:
        return step_size_args(value, n_chains, device)
    except ValueError as e:
        raise ValueError(str(e).replace("step_size", name)) from None


def _batch_args(position, step_size, temperature, name: str = "position", step_size_name: str = "step_size"):
    """-> contiguous device position, (eps, per-chain eps), (T, per-chain T).  Shapes are checked before the device,
    so that a wrong-length per-chain argument is a ``ValueError`` wherever the tensors live."""
    if not isinstance(position, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(position)}")
    if position.ndim != 2:
        raise ValueError(f"{name} must be (n_chains, dim), got {tuple(position.shape)}")
    n = position.shape[0]
    eps = _per_chain(step_size, n, position.device, step_size_name)
    temp = _per_chain(temperature, n, position.device, "temperature")
    return check_batch(position, name), eps, temp


def _like(x, q, name: str):
    x = check_batch(x, name)
    if x.shape != q.shape or x.device != q.device:
        raise ValueError(f"{name} must be {tuple(q.shape)} on {q.device}, got {tuple(x.shape)} on {x.device}")
    return x


def check_friction(step_size, alpha: float, beta: float) -> None:
    """The noise scale ``sqrt(step_size * T * (2 alpha - step_size beta))`` of ``sghmc`` / ``sgnht`` needs
    ``2 alpha >= step_size beta``; the reference silently produces NaN.  Checked for a float ``step_size`` only:
    per-chain tensors are not read back."""
    if isinstance(step_size, torch.Tensor) and (step_size.ndim != 0 or step_size.is_cuda):
        return
    if 2.0 * float(alpha) - float(step_size) * float(beta) < 0.0:
        raise ValueError(f"2 * alpha - step_size * beta must not be negative (alpha = {alpha}, beta = {beta}, "
                         f"step_size = {float(step_size)}): the noise scale would be NaN")


def estimate_gradient(grad_estimator, position, minibatch):
    """Call the user's ``grad_estimator(position, minibatch)`` and normalise its output to contiguous fp32 ``(N, D)``
    on the position's device.  ``minibatch`` is handed on untouched."""
    g = grad_estimator(position, minibatch)
    if not isinstance(g, torch.Tensor) or g.shape != position.shape:
        raise ValueError(f"grad_estimator must return a tensor of shape {tuple(position.shape)}, got "
                         f"{tuple(g.shape) if isinstance(g, torch.Tensor) else type(g)}")
    if g.device != position.device:
        raise RuntimeError(f"grad_estimator returned a gradient on {g.device} for positions on {position.device}")
    if g.dtype != torch.float32:
        g = g.float()
    return g.detach().contiguous()


def overdamped_langevin():
    """blackjax/sgmcmc/diffusions.py ``overdamped_langevin``:
    ``q + step_size * grad + sqrt(2 * temperature * step_size) * normal(kc, (D,))``."""

    def one_step(rng_key, position, logdensity_grad, step_size, temperature=1.0, *, chain_offset: int = 0):
        q, (eps, eps_pc), (temp, temp_pc) = _batch_args(position, step_size, temperature)
        g = _like(logdensity_grad, q, "logdensity_grad")
        N, D = q.shape
        k0, k1, fold = key_spec(rng_key)
        q_new = torch.empty_like(q)
        _lib.call("bjx_sgld_step", _lib.current_stream(), k0, k1, int(chain_offset), fold, N, D, eps,
                  _lib.ptr(eps_pc), temp, _lib.ptr(temp_pc), q.data_ptr(), g.data_ptr(), q_new.data_ptr())
        return q_new

    return one_step


def sghmc(alpha: float = 0.01, beta: float = 0.0):
    """blackjax/sgmcmc/diffusions.py ``sghmc``, as integration step ``step_index`` = l of a transition:
    ``q + step_size * p`` and ``(1 - alpha * step_size) * p + step_size * grad + s * normal(split(kc, L)[l], (D,))``
    with ``s = sqrt(step_size * temperature * (2 alpha - step_size * beta))``.

    ``momentum=None``: the momentum is the transition's refresh ``normal(kc, (D,))``, drawn inside the launch.
    ``logdensity_grad=None``: only the new position is computed and ``(position, None)`` returned (the last step of a
    transition, whose momentum the sampler drops)."""
    alpha, beta = float(alpha), float(beta)

    def one_step(rng_key, position, momentum, logdensity_grad, step_size, temperature=1.0, *,
                 chain_offset: int = 0, step_index: int = 0):
        check_friction(step_size, alpha, beta)
        q, (eps, eps_pc), (temp, temp_pc) = _batch_args(position, step_size, temperature)
        p = None if momentum is None else _like(momentum, q, "momentum")
        g = None if logdensity_grad is None else _like(logdensity_grad, q, "logdensity_grad")
        N, D = q.shape
        k0, k1, fold = key_spec(rng_key)
        q_new = torch.empty_like(q)
        p_new = None if g is None else torch.empty_like(q)
        _lib.call("bjx_sghmc_step", _lib.current_stream(), k0, k1, int(chain_offset), fold, N, D, int(step_index),
                  alpha, beta, eps, _lib.ptr(eps_pc), temp, _lib.ptr(temp_pc), q.data_ptr(), _lib.ptr(p),
                  _lib.ptr(g), q_new.data_ptr(), _lib.ptr(p_new))
        return q_new, p_new

    return one_step


def sgnht(alpha: float = 0.01, beta: float = 0.0):
    """blackjax/sgmcmc/diffusions.py ``sgnht``: ``q + step_size * p``,
    ``p - step_size * xi * p + step_size * grad + s * normal(kc, (D,))`` with ``s`` as for ``sghmc``, and
    ``xi + step_size * (mean(p_new ** 2) - temperature)``; returns ``(position, momentum, xi)``."""
    alpha, beta = float(alpha), float(beta)

    def one_step(rng_key, position, momentum, xi, logdensity_grad, step_size, temperature=1.0, *,
                 chain_offset: int = 0):
        check_friction(step_size, alpha, beta)
        q, (eps, eps_pc), (temp, temp_pc) = _batch_args(position, step_size, temperature)
        p = _like(momentum, q, "momentum")
        g = _like(logdensity_grad, q, "logdensity_grad")
        x = check_batch(xi, "xi")
        N, D = q.shape
        if x.shape != (N,) or x.device != q.device:
            raise ValueError(f"xi must be ({N},) on {q.device}, got {tuple(x.shape)} on {x.device}")
        k0, k1, fold = key_spec(rng_key)
        q_new, p_new, x_new = torch.empty_like(q), torch.empty_like(q), torch.empty_like(x)
        _lib.call("bjx_sgnht_step", _lib.current_stream(), k0, k1, int(chain_offset), fold, N, D, alpha, beta, eps,
                  _lib.ptr(eps_pc), temp, _lib.ptr(temp_pc), q.data_ptr(), p.data_ptr(), x.data_ptr(), g.data_ptr(),
                  q_new.data_ptr(), p_new.data_ptr(), x_new.data_ptr())
        return q_new, p_new, x_new

    return one_step
