"""Batched contour stochastic gradient Langevin dynamics on MI355X behind the ``blackjax.csgld`` API surface.

Mirrors blackjax/sgmcmc/csgld.py: ``ContourSGLDState``, ``init``, ``build_kernel`` and ``as_top_level_api``.  Every
chain keeps its own estimate of the energy histogram, ``energy_pdf`` (N, M), and the index of the bin its energy last
fell into, ``energy_idx`` (N,) int32.  The gradient is scaled by ``1 + zeta T (log pdf[i] - log pdf[i - 1]) /
energy_gap``, the slope of that histogram at the chain's bin, which flattens the energy landscape and lets a chain
leave a mode; the histogram is then moved towards the bin of the energy at the NEW position by stochastic
approximation.

A transition is, in this order: the user's ``gradient_estimator(position, minibatch)`` at the old position;
``bjx_csgld_step`` (the multiplier, the noise draw and the Langevin update: the scaled gradient is never stored);
the user's ``logdensity_estimator(new position, minibatch)``; ``bjx_csgld_update`` (bin index and histogram update in
one pass over the (N, M) array).  Both launches are declared in include/bjx_hip.h under "SGMCMC"; nothing is read
back from the device and every output is out of place.  Neither estimator is traced: the minibatch changes every step.

The chain axis is native; chain ``i`` reproduces the reference's single-chain step made with
``jax.random.split(rng_key, N)[chain_offset + i]``, the chain key drawing the noise unsplit.  ``step_size_diff``,
``step_size_stoch`` and ``temperature`` are Python floats or per-chain ``(N,)`` device tensors and arrive with every
call; ``zeta``, ``energy_gap`` and ``min_energy`` are kernel arguments and compile nothing.  A non-positive histogram
entry gives a NaN row, as in the reference.  Like every RNG-dependent part of the package, parity with a real JAX run
is unpinned; the arithmetic is held against a NumPy restatement of the reference
(tests/csgld_restatement.py).
"""
from __future__ import annotations

from typing import Callable, NamedTuple

import torch

from .. import _lib
from .._util import check_batch
from ..base import SamplingAlgorithm
from ..random import key_spec
from . import diffusions

__all__ = ["ContourSGLDState", "init", "build_kernel", "as_top_level_api", "langevin_step",
           "update_energy_histogram"]


class ContourSGLDState(NamedTuple):
    """blackjax/sgmcmc/csgld.py ``ContourSGLDState``, batched: (N, D) fp32, (N, M) fp32, (N,) int32."""

    position: torch.Tensor
    energy_pdf: torch.Tensor
    energy_idx: torch.Tensor


def init(position: torch.Tensor, num_partitions=512) -> ContourSGLDState:
    """blackjax/sgmcmc/csgld.py ``init``: every chain starts from the histogram ``(M - j) / (M (M + 1) / 2)`` (one
    fp32 division per entry) with its index on the last bin, ``M - 1``."""
    M = int(num_partitions)
    if M < 2:
        raise ValueError(f"num_partitions must be at least 2, got {num_partitions}")
    if isinstance(position, torch.Tensor) and position.ndim != 2:
        raise ValueError(f"position must be (n_chains, dim), got {tuple(position.shape)}")
    position = check_batch(position, "position")
    N, dev = position.shape[0], position.device
    # divided on the host, element by element: an IEEE fp32 division, where a device division by a scalar may be a
    # multiplication by its reciprocal
    row = torch.arange(M, 0, -1, dtype=torch.float32) / torch.full((M,), float(M * (M + 1) // 2), dtype=torch.float32)
    energy_pdf = row.to(dev).expand(N, M).contiguous()
    energy_idx = torch.full((N,), M - 1, dtype=torch.int32, device=dev)
    return ContourSGLDState(position, energy_pdf, energy_idx)


def _check_gap(energy_gap) -> float:
    if not float(energy_gap) > 0.0:
        raise ValueError(f"energy_gap must be positive, got {energy_gap}")
    return float(energy_gap)


def _check_histogram(energy_pdf, n_chains: int):
    """Shape and dtype of an (N, M >= 2) fp32 histogram, checked before the device, so that a wrong one is a
    ``ValueError`` wherever the tensors live."""
    if not isinstance(energy_pdf, torch.Tensor):
        raise TypeError(f"energy_pdf must be a torch.Tensor, got {type(energy_pdf)}")
    if energy_pdf.ndim != 2 or energy_pdf.shape[0] != n_chains or energy_pdf.shape[1] < 2:
        raise ValueError(f"energy_pdf must be ({n_chains}, num_partitions >= 2), got {tuple(energy_pdf.shape)}")
    if energy_pdf.dtype != torch.float32:
        raise ValueError(f"energy_pdf must be float32, got {energy_pdf.dtype}")


def _check_index(energy_idx, n_chains: int):
    if not isinstance(energy_idx, torch.Tensor):
        raise TypeError(f"energy_idx must be a torch.Tensor, got {type(energy_idx)}")
    if energy_idx.shape != (n_chains,) or energy_idx.dtype != torch.int32:
        raise ValueError(f"energy_idx must be int32 ({n_chains},), got {energy_idx.dtype} {tuple(energy_idx.shape)}")


def _on(x, device, name: str):
    if x.device != device:
        raise ValueError(f"{name} must be on {device}, got {x.device}")
    return x.contiguous()


def langevin_step(rng_key, position, logdensity_grad, energy_pdf, energy_idx, step_size_diff, temperature=1.0, *,
                  zeta: float = 1.0, energy_gap: float = 10.0, chain_offset: int = 0):
    """The position half of a transition, one launch of ``bjx_csgld_step``:
    ``q + step_size_diff * (m * grad) + sqrt(2 * temperature * step_size_diff) * normal(kc, (D,))`` with the per-chain
    ``m = 1 + zeta * temperature * (log pdf[i] - log pdf[i - 1]) / energy_gap``.  ``energy_idx`` is clamped into
    ``[1, M - 1]`` by the kernel.  Returns the new position."""
    gap = _check_gap(energy_gap)
    if isinstance(position, torch.Tensor) and position.ndim == 2:
        _check_histogram(energy_pdf, position.shape[0])
        _check_index(energy_idx, position.shape[0])
    q, (eps, eps_pc), (temp, temp_pc) = diffusions._batch_args(position, step_size_diff, temperature,
                                                               step_size_name="step_size_diff")
    g = diffusions._like(logdensity_grad, q, "logdensity_grad")
    N, D = q.shape
    pdf = _on(check_batch(energy_pdf, "energy_pdf"), q.device, "energy_pdf")
    idx = _on(energy_idx, q.device, "energy_idx")
    k0, k1, fold = key_spec(rng_key)
    q_new = torch.empty_like(q)
    _lib.call("bjx_csgld_step", _lib.current_stream(), k0, k1, int(chain_offset), fold, N, D, pdf.shape[1],
              float(zeta), gap, eps, _lib.ptr(eps_pc), temp, _lib.ptr(temp_pc), q.data_ptr(), g.data_ptr(),
              pdf.data_ptr(), idx.data_ptr(), q_new.data_ptr())
    return q_new


def update_energy_histogram(logdensity, energy_pdf, step_size_stoch, *, zeta: float = 1.0, energy_gap: float = 10.0,
                            min_energy: float = 0.0):
    """The histogram half of a transition, one launch of ``bjx_csgld_update``: the bin
    ``i = clamp(floor((-logdensity - min_energy) / energy_gap + 1), 1, M - 1)`` of every chain's energy and
    ``pdf + step_size_stoch * pdf[i] ** zeta * (e_i - pdf)``.  Returns ``(energy_pdf, energy_idx)``."""
    gap = _check_gap(energy_gap)
    if not isinstance(logdensity, torch.Tensor):
        raise TypeError(f"logdensity must be a torch.Tensor, got {type(logdensity)}")
    if logdensity.ndim != 1:
        raise ValueError(f"logdensity must be (n_chains,), got {tuple(logdensity.shape)}")
    N = logdensity.shape[0]
    _check_histogram(energy_pdf, N)
    eps, eps_pc = diffusions._per_chain(step_size_stoch, N, logdensity.device, "step_size_stoch")
    ld = check_batch(logdensity, "logdensity")
    pdf = _on(check_batch(energy_pdf, "energy_pdf"), ld.device, "energy_pdf")
    pdf_new = torch.empty_like(pdf)
    idx_new = torch.empty(N, dtype=torch.int32, device=ld.device)
    _lib.call("bjx_csgld_update", _lib.current_stream(), N, pdf.shape[1], float(zeta), gap, float(min_energy), eps,
              _lib.ptr(eps_pc), ld.data_ptr(), pdf.data_ptr(), pdf_new.data_ptr(), idx_new.data_ptr())
    return pdf_new, idx_new


def estimate_logdensity(logdensity_estimator, position, minibatch):
    """Call the user's ``logdensity_estimator(position, minibatch)`` and normalise its output to contiguous fp32
    ``(N,)`` on the position's device, as ``diffusions.estimate_gradient`` does for the gradient."""
    ld = logdensity_estimator(position, minibatch)
    if not isinstance(ld, torch.Tensor) or ld.shape != position.shape[:1]:
        raise ValueError(f"logdensity_estimator must return a tensor of shape {tuple(position.shape[:1])}, got "
                         f"{tuple(ld.shape) if isinstance(ld, torch.Tensor) else type(ld)}")
    if ld.device != position.device:
        raise RuntimeError(f"logdensity_estimator returned a log-density on {ld.device} for positions on "
                           f"{position.device}")
    if ld.dtype != torch.float32:
        ld = ld.float()
    return ld.detach().contiguous()


def build_kernel(num_partitions=512, energy_gap=10, min_energy=0):
    """blackjax/sgmcmc/csgld.py ``build_kernel``."""
    M = int(num_partitions)
    if M < 2:
        raise ValueError(f"num_partitions must be at least 2, got {num_partitions}")
    gap, floor_energy = _check_gap(energy_gap), float(min_energy)

    def kernel(rng_key, state: ContourSGLDState, logdensity_estimator: Callable, gradient_estimator: Callable,
               minibatch, step_size_diff, step_size_stoch, zeta=1, temperature=1.0, *,
               chain_offset: int = 0) -> ContourSGLDState:
        position, energy_pdf, energy_idx = state
        zeta = float(zeta)
        if isinstance(position, torch.Tensor) and position.ndim == 2:  # every shape before the device
            N = position.shape[0]
            _check_histogram(energy_pdf, N)
            _check_index(energy_idx, N)
            if energy_pdf.shape[1] != M:
                raise ValueError(f"state.energy_pdf must be ({N}, {M}), got {tuple(energy_pdf.shape)}")
            diffusions._per_chain(step_size_stoch, N, position.device, "step_size_stoch")
        q, _, _ = diffusions._batch_args(position, step_size_diff, temperature, "state.position",
                                         step_size_name="step_size_diff")
        g = diffusions.estimate_gradient(gradient_estimator, q, minibatch)
        q_new = langevin_step(rng_key, q, g, energy_pdf, energy_idx, step_size_diff, temperature, zeta=zeta,
                              energy_gap=gap, chain_offset=chain_offset)
        ld = estimate_logdensity(logdensity_estimator, q_new, minibatch)
        pdf_new, idx_new = update_energy_histogram(ld, energy_pdf, step_size_stoch, zeta=zeta, energy_gap=gap,
                                                   min_energy=floor_energy)
        return ContourSGLDState(q_new, pdf_new, idx_new)

    return kernel


def as_top_level_api(logdensity_estimator: Callable, gradient_estimator: Callable, zeta=1, num_partitions=512,
                     energy_gap=100, min_energy=0, *, chain_offset: int = 0) -> SamplingAlgorithm:
    """blackjax/sgmcmc/csgld.py ``as_top_level_api``: ``init(position, rng_key=None)``,
    ``step(rng_key, state, minibatch, step_size_diff, step_size_stoch, temperature=1.0)``."""
    kernel = build_kernel(num_partitions, energy_gap, min_energy)

    def init_fn(position, rng_key=None):
        del rng_key
        return init(position, num_partitions)

    def step_fn(rng_key, state, minibatch, step_size_diff, step_size_stoch, temperature=1.0):
        return kernel(rng_key, state, logdensity_estimator, gradient_estimator, minibatch, step_size_diff,
                      step_size_stoch, zeta, temperature, chain_offset=chain_offset)

    return SamplingAlgorithm(init_fn, step_fn)
