"""blackjax/smc/tuning/from_particles.py: strategies that tune the move from the particle cloud.

Means and standard deviations come from ``bjx_smc_particle_moments`` (include/bjx_hip.h "SMC"): fp64 accumulators
over fixed row tiles, merged in order, each result rounded once; reproducible bit for bit and never read back.
"""
from __future__ import annotations

import torch

from .. import base
from ... import _lib

__all__ = ["particles_means", "particles_stds", "particles_covariance_matrix", "mass_matrix_from_particles",
           "particles_as_rows", "MOMENTS_TILE"]

MOMENTS_TILE = 256  # rows per workgroup of the moments kernel (bjx_smc_moments_tile())


def particles_as_rows(particles) -> torch.Tensor:
    """blackjax/smc/tuning/from_particles.py ``particles_as_rows``: the particles as an ``(N, D)`` matrix.  Here
    they already are one (pytrees of particles are out of scope): the identity."""
    return base.check_particles(particles)


def _moments(particles, want_std: bool):
    x = base.check_particles(particles)
    n, d = x.shape
    nbytes = _lib.load().bjx_smc_particle_moments_workspace_bytes(n, d)
    if nbytes == 0:
        raise ValueError(f"particle moments support at most 2**24 particles of at most 2**20 columns, got {n} x {d}")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
    mean = torch.empty(d, dtype=torch.float32, device=x.device)
    std = torch.empty(d, dtype=torch.float32, device=x.device) if want_std else None
    _lib.call("bjx_smc_particle_moments", _lib.current_stream(), n, d, x.data_ptr(), ws.data_ptr(), mean.data_ptr(),
              std.data_ptr() if want_std else None)
    return x, mean, std, ws[-2 * d:-d]


def particles_means(particles) -> torch.Tensor:
    """``(D,)`` column means (``jnp.mean(particles_as_rows(particles), axis=0)``)."""
    return _moments(particles, False)[1]


def particles_stds(particles) -> torch.Tensor:
    """``(D,)`` column standard deviations with ddof 0 (``jnp.std(..., axis=0)``); 0 for a single particle."""
    return _moments(particles, True)[2]


def particles_covariance_matrix(particles) -> torch.Tensor:
    """``(D, D)`` covariance with ddof 1 (``jnp.cov(particles_as_rows(particles), rowvar=False)``).  The rows are
    centred with the kernel's fp64 means; the product is one fp32 GEMM."""
    n = base.check_particles(particles).shape[0]
    if n < 2:
        raise ValueError("the covariance of the particles needs at least two of them")
    x, _, _, mean64 = _moments(particles, False)
    c = (x.double() - mean64).float()
    return (c.t() @ c) / float(n - 1)


def mass_matrix_from_particles(particles) -> torch.Tensor:
    """blackjax/smc/tuning/from_particles.py ``mass_matrix_from_particles``: the diagonal MASS matrix
    ``1 / stds**2``, ``(D,)``.  The samplers of this package take ``inverse_mass_matrix=``, which wants
    ``particles_stds(particles)**2``, not this."""
    stds = particles_stds(particles)
    return 1.0 / (stds * stds)
