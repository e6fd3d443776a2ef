"""Systematic, stratified, multinomial and residual resampling behind ``blackjax.smc.resampling``.

Mirrors blackjax/smc/resampling.py ``systematic`` and ``stratified`` (``searchsorted`` of the positions
``(i + u_i) / num_samples`` in the cumulative weights, clipped to ``N - 1``), ``multinomial`` (the positions are
``_sorted_uniforms``) and ``residual`` (``floor(num_samples * w_j)`` copies for certain, a permuted multinomial draw
of the fractional parts for the rest).  ``num_samples`` need not equal ``N``: persistent sampling
(``blackjax_amd.smc.persistent_sampling``) draws ``N`` ancestors from the ``i * N`` weights of its persistent set and
waste-free SMC (``blackjax_amd.smc.waste_free``) draws ``N / p``.

The cumulative weights are held in 2^-62 fixed point (``bjx_smc_resample``, include/bjx_hip.h "SMC"): integer sums
do not depend on how the prefix scan is tiled, so the ancestors are reproducible bit for bit
(tests/smc_restatement.py).  Positions are formed in fp32, hence ``num_samples <= 2**24`` and ``N <= 2**24``.  The
sorted uniforms of ``multinomial`` / ``residual`` come from an INTEGER prefix sum of fixed-point exponentials
(``bjx_smc_resample_sorted``; tests/smc_extra_restatement.py), for the same reason.
"""
from __future__ import annotations

import torch

from .. import _lib
from .._util import check_batch
from ..random import key_words, permutation, split

__all__ = ["systematic", "stratified", "multinomial", "residual", "SCAN_TILE", "MAX_PARTICLES"]

SCAN_TILE = 1024  # items per workgroup of the prefix scan (bjx_smc_scan_tile())
MAX_PARTICLES = 1 << 24


def _checked(weights, num_samples, validate: bool):
    w = check_batch(weights, "weights")
    if w.ndim != 1:
        raise ValueError(f"weights must be (n_particles,), got {tuple(w.shape)}")
    n, m = int(w.shape[0]), int(num_samples)
    if n < 1:
        raise ValueError("resampling needs at least one particle")
    if n > MAX_PARTICLES or not 0 <= m <= MAX_PARTICLES:
        raise ValueError(f"resampling supports at most 2**24 particles and samples (positions are fp32), got "
                         f"N = {n}, num_samples = {m}")
    if validate:  # the one host read of a direct call; the SMC step, whose weights are its own, skips it
        total, smallest = torch.stack([w.sum(dtype=torch.float64), w.min().double()]).tolist()
        if not (smallest >= 0.0 and abs(total - 1.0) <= 1e-3):
            raise ValueError(f"weights must be non-negative and sum to 1 (sum = {total}, min = {smallest})")
    return w, n, m


def _resample(rng_key, weights, num_samples, stratified: bool, validate: bool) -> torch.Tensor:
    w, n, m = _checked(weights, num_samples, validate)
    k0, k1 = key_words(rng_key)
    ws = torch.empty(_lib.load().bjx_smc_resample_workspace_bytes(n) // 8, dtype=torch.int64, device=w.device)
    ancestors = torch.empty(m, dtype=torch.int32, device=w.device)
    _lib.call("bjx_smc_resample", _lib.current_stream(), k0, k1, 1 if stratified else 0, n, m, w.data_ptr(),
              ws.data_ptr(), ancestors.data_ptr())
    return ancestors


def systematic(rng_key, weights, num_samples) -> torch.Tensor:
    """blackjax/smc/resampling.py ``systematic``: one uniform shared by all positions.  ``weights``: normalised
    float32 ``(N,)`` device tensor; returns ``(num_samples,)`` int32 ancestors on the device."""
    return _resample(rng_key, weights, num_samples, False, True)


def stratified(rng_key, weights, num_samples) -> torch.Tensor:
    """blackjax/smc/resampling.py ``stratified``: one uniform per position."""
    return _resample(rng_key, weights, num_samples, True, True)


MULTINOMIAL, RESIDUAL = 0, 1  # BJX_SMC_MULTINOMIAL, BJX_SMC_RESIDUAL


def _resample_sorted(rng_key, weights, num_samples, mode: int, validate: bool) -> torch.Tensor:
    w, n, m = _checked(weights, num_samples, validate)
    ancestors = torch.empty(m, dtype=torch.int32, device=w.device)
    if m == 0:
        return ancestors
    perm_ptr = None
    if mode == RESIDUAL:  # the permutation depends on the key alone: formed on the host, uploaded
        keys = split(rng_key, 2)
        rng_key = keys[0]
        perm = torch.as_tensor(permutation(keys[1], m).astype("int32"), device=w.device)
        perm_ptr = perm.data_ptr()
    k0, k1 = key_words(rng_key)
    ws = torch.empty(_lib.load().bjx_smc_resample_sorted_workspace_bytes(n, m) // 8, dtype=torch.int64,
                     device=w.device)
    _lib.call("bjx_smc_resample_sorted", _lib.current_stream(), k0, k1, mode, n, m, w.data_ptr(), perm_ptr,
              ws.data_ptr(), ancestors.data_ptr())
    return ancestors


def multinomial(rng_key, weights, num_samples) -> torch.Tensor:
    """blackjax/smc/resampling.py ``multinomial``: ``searchsorted(cumsum(w), _sorted_uniforms(key, num_samples))``,
    non-decreasing ancestors.  The sorted uniforms are ``Z_i / Z_M`` with ``Z`` the integer prefix sum of
    ``floor(e_k * 2**24)``, ``e_k = -log1p(-u_k)`` (include/bjx_hip.h "SMC").  Deliberate deviation: the reference
    takes ``-log(u_k)``, which is ``inf`` for a draw of exactly 0; ``1 - u`` is as uniform as ``u`` and keeps every
    exponential finite."""
    return _resample_sorted(rng_key, weights, num_samples, MULTINOMIAL, True)


def residual(rng_key, weights, num_samples) -> torch.Tensor:
    """blackjax/smc/resampling.py ``residual``: particle ``j`` appears ``floor(num_samples * w_j)`` times for
    certain (the first ``S`` positions, in order); the other ``num_samples - S`` positions hold the matching entries
    of a permuted multinomial draw of ``num_samples`` from the fractional parts.  ``S`` stays on the device."""
    return _resample_sorted(rng_key, weights, num_samples, RESIDUAL, True)


# what the SMC steps call: the weights are the output of bjx_smc_reweight, so the normalisation check (a host read)
# is skipped
systematic._bjx_trusted = lambda rng_key, weights, num_samples: _resample(rng_key, weights, num_samples, False, False)
stratified._bjx_trusted = lambda rng_key, weights, num_samples: _resample(rng_key, weights, num_samples, True, False)
multinomial._bjx_trusted = lambda rng_key, weights, num_samples: _resample_sorted(rng_key, weights, num_samples,
                                                                                 MULTINOMIAL, False)
residual._bjx_trusted = lambda rng_key, weights, num_samples: _resample_sorted(rng_key, weights, num_samples,
                                                                              RESIDUAL, False)
