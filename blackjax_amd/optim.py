"""Gradient transformations: for the ChEES trajectory-length optimiser (one host scalar) and for ``meanfield_vi``
(device tensors).

The reference takes any ``optax.GradientTransformation`` (chees_adaptation.py:741, 474-481) and only
ever applies it to ONE scalar, ``log(trajectory_length)``.  optax is a third-party dependency that
is not part of the reference tree (pinned 0.2.8, uv.lock:2197-2198); ``adam`` and ``sgd`` restate its
published update rules for a scalar parameter, in fp32 operation by operation (pow in fp64, rounded
once).  Any object with ``init(params) -> state`` and ``update(grad, state, params) -> (update, state)``
can be passed instead.

``meanfield_vi`` applies the same transformations to its ``(mu, rho)`` parameters: when ``init`` / ``update`` receive
a float32 device tensor, or a tuple of them, the moments are device tensors of the same shapes, ``count`` stays a
host integer, and an update is one launch per leaf (``bjx_optim_adam`` / ``bjx_optim_sgd``, include/bjx_hip.h "VI")
that mirrors the scalar code below operation by operation, the bias corrections formed on the host exactly as there.
Nothing is read back.  Host scalars take the scalar code, unchanged.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

f32 = np.float32
f64 = np.float64


class ScaleByAdamState(NamedTuple):
    count: int
    mu: np.float32
    nu: np.float32


def _is_leaf(x) -> bool:
    import torch

    return isinstance(x, torch.Tensor) and x.is_cuda


def _is_device(tree) -> bool:
    """A device tensor, or a tuple / list of them: the trees the device path takes."""
    if isinstance(tree, (tuple, list)):
        return len(tree) > 0 and all(_is_leaf(v) for v in tree)
    return _is_leaf(tree)


def _leaves(tree) -> list:
    return list(tree) if isinstance(tree, (tuple, list)) else [tree]


def _like(tree, leaves):
    """``leaves`` in the structure of ``tree``."""
    return tuple(leaves) if isinstance(tree, (tuple, list)) else leaves[0]


def _leaf(x, name: str, like=None):
    """``x`` as a contiguous fp32 device tensor, of ``like``'s shape and device when given."""
    import torch

    if not _is_leaf(x) or x.dtype != torch.float32:
        raise TypeError(f"{name} must be a float32 device tensor, got "
                        f"{(x.dtype, x.device) if isinstance(x, torch.Tensor) else type(x)}")
    if like is not None and (x.shape != like.shape or x.device != like.device):
        raise ValueError(f"{name} must have shape {tuple(like.shape)} on {like.device}, got {tuple(x.shape)} on "
                         f"{x.device}")
    return x.contiguous()


class _Adam:
    def __init__(self, learning_rate, b1, b2, eps, eps_root):
        self.learning_rate, self.b1, self.b2 = float(learning_rate), float(b1), float(b2)
        self.eps, self.eps_root = float(eps), float(eps_root)

    def init(self, params):
        if _is_device(params):
            import torch

            def zeros():
                return _like(params, [torch.zeros_like(_leaf(p, "params")) for p in _leaves(params)])

            return ScaleByAdamState(0, zeros(), zeros())
        del params
        return ScaleByAdamState(0, f32(0.0), f32(0.0))

    def _update_device(self, grad, state):
        """``update`` on device tensors: one ``bjx_optim_adam`` launch per leaf, the scalars formed as below."""
        import torch

        from . import _lib

        b1, b2 = f32(self.b1), f32(self.b2)
        count = state.count + 1
        c1 = f32(f32(1.0) - f32(np.power(f64(b1), f64(count))))
        c2 = f32(f32(1.0) - f32(np.power(f64(b2), f64(count))))
        scalars = [float(v) for v in (b1, b2, f32(1.0 - self.b1), f32(1.0 - self.b2), c1, c2, f32(self.eps),
                                      f32(self.eps_root), f32(-self.learning_rate))]
        gs, mus, nus = _leaves(grad), _leaves(state.mu), _leaves(state.nu)
        if not len(gs) == len(mus) == len(nus):
            raise ValueError(f"the optimiser state holds {len(mus)} leaves for {len(gs)} gradients")
        us, mus_new, nus_new = [], [], []
        for g, mu, nu in zip(gs, mus, nus):
            g = _leaf(g, "grad")
            mu, nu = _leaf(mu, "state.mu", g), _leaf(nu, "state.nu", g)
            u, mu_new, nu_new = torch.empty_like(g), torch.empty_like(g), torch.empty_like(g)
            with torch.cuda.device(g.device):
                _lib.call("bjx_optim_adam", _lib.current_stream(), g.numel(), *scalars, g.data_ptr(), mu.data_ptr(),
                          nu.data_ptr(), mu_new.data_ptr(), nu_new.data_ptr(), u.data_ptr())
            us.append(u), mus_new.append(mu_new), nus_new.append(nu_new)
        return _like(grad, us), ScaleByAdamState(count, _like(grad, mus_new), _like(grad, nus_new))

    def update(self, grad, state, params=None):
        """scale_by_adam: ``mu = (1-b1) g + b1 mu``, ``nu = (1-b2) g^2 + b2 nu``, bias correction
        ``m / (1 - b^count)``, ``u = mu_hat / (sqrt(nu_hat + eps_root) + eps)``; then ``-lr * u``."""
        del params
        if _is_device(grad):
            return self._update_device(grad, state)
        g = f32(grad)
        b1, b2 = f32(self.b1), f32(self.b2)
        mu = f32(f32(f32(1.0 - self.b1) * g) + f32(b1 * state.mu))
        nu = f32(f32(f32(1.0 - self.b2) * f32(g * g)) + f32(b2 * state.nu))
        count = state.count + 1
        c1 = f32(f32(1.0) - f32(np.power(f64(b1), f64(count))))
        c2 = f32(f32(1.0) - f32(np.power(f64(b2), f64(count))))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            mu_hat = f32(mu / c1)
            nu_hat = f32(nu / c2)
            u = f32(mu_hat / f32(f32(np.sqrt(f32(nu_hat + f32(self.eps_root)))) + f32(self.eps)))
            return f32(f32(-self.learning_rate) * u), ScaleByAdamState(count, mu, nu)


def adam(learning_rate, b1=0.9, b2=0.999, eps=1e-8, eps_root=0.0):
    """``optax.adam`` for one scalar parameter, or for device tensors (see the module docstring)."""
    return _Adam(learning_rate, b1, b2, eps, eps_root)


class _SGD:
    def __init__(self, learning_rate):
        self.learning_rate = float(learning_rate)

    def init(self, params):
        del params
        return ()

    def update(self, grad, state, params=None):
        del params
        if _is_device(grad):
            import torch

            from . import _lib

            us = []
            for g in _leaves(grad):
                g = _leaf(g, "grad")
                u = torch.empty_like(g)
                with torch.cuda.device(g.device):
                    _lib.call("bjx_optim_sgd", _lib.current_stream(), g.numel(), float(f32(-self.learning_rate)),
                              g.data_ptr(), u.data_ptr())
                us.append(u)
            return _like(grad, us), state
        return f32(f32(-self.learning_rate) * f32(grad)), state


def sgd(learning_rate):
    """``optax.sgd`` (no momentum) for one scalar parameter, or for device tensors."""
    return _SGD(learning_rate)
