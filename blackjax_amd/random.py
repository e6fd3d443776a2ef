"""Host-side threefry key helpers with ``jax.random`` semantics.

Keys are ``uint32[2]`` (jax.random key data).  Device kernels derive per-chain and
per-element streams themselves from a key passed by value; the host only ever
splits a run key into per-step keys (blackjax/util.py:203,
adaptation/staged_adaptation.py:868), which is done by the C-ABI host function
``bjx_keys_split``.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

__all__ = ["key", "PRNGKey", "split", "fold_in", "uniform", "permutation", "key_words", "ChainMajorKey", "key_spec", "chain_normal"]


def key(seed: int) -> np.ndarray:
    """jax.random.key(seed) key data: ``[seed >> 32, seed & 0xffffffff]``."""
    seed = int(seed)
    return np.array([(seed >> 32) & 0xFFFFFFFF, seed & 0xFFFFFFFF], dtype=np.uint32)


PRNGKey = key


def key_words(rng_key) -> tuple[int, int]:
    """Normalise an int seed / array-like uint32[2] key to two Python ints."""
    if isinstance(rng_key, (int, np.integer)):
        rng_key = key(int(rng_key))
    if hasattr(rng_key, "detach"):  # torch tensor (must be host data: no device sync here)
        if rng_key.is_cuda:
            raise ValueError("rng_key must live on the host (uint32[2]); got a device tensor")
        rng_key = rng_key.detach().numpy()
    k = np.asarray(rng_key)
    if k.shape != (2,):
        raise ValueError(f"rng_key must be an int seed or have shape (2,), got {k.shape}")
    return int(k[0]) & 0xFFFFFFFF, int(k[1]) & 0xFFFFFFFF


def split(rng_key, num: int = 2, offset: int = 0) -> np.ndarray:
    """jax.random.split(key, num) -> (num, 2) uint32 (rows offset..offset+num of a larger split)."""
    k0, k1 = key_words(rng_key)
    out = np.empty((int(num), 2), dtype=np.uint32)
    _lib.call("bjx_keys_split", k0, k1, int(num), int(offset),
              out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    return out


def fold_in(rng_key, data: int) -> np.ndarray:
    """jax.random.fold_in(key, data) == split(key, .)[data] for threefry-partitionable keys."""
    return split(rng_key, 1, offset=int(data) & 0xFFFFFFFF)[0]


def uniform(rng_key) -> np.float32:
    """jax.random.uniform(key, (), float32) on the host: 23 mantissa bits of
    ``random_bits(key, 32, ())`` = the xor of the two threefry output words at counter 0."""
    w = split(rng_key, 1)[0]
    bits = np.uint32(w[0] ^ w[1])
    f = (np.array([(bits >> np.uint32(9)) | np.uint32(0x3F800000)], np.uint32).view(np.float32)[0]
         - np.float32(1.0))
    return np.float32(max(np.float32(0.0), f))


def permutation(rng_key, n: int) -> np.ndarray:
    """``jax.random.permutation(key, n)`` (jax/_src/random.py::_shuffle): ceil(3 ln n / ln(2^32 - 1))
    rounds of a stable sort by fresh 32-bit keys, ``key, subkey = split(key)`` per round."""
    x = np.arange(n, dtype=np.int64)
    rounds = int(np.ceil(3 * np.log(max(1, n)) / np.log(float(2**32 - 1))))
    key = rng_key
    for _ in range(rounds):
        key, sub = split(key, 2)
        words = split(sub, n)  # random_bits(sub, 32, (n,))[i] = xor of the words of child i
        bits = words[:, 0] ^ words[:, 1]
        x = x[np.argsort(bits, kind="stable")]
    return x


class ChainMajorKey:
    """Step ``t`` of a chain-major run: chain ``i`` uses
    ``split(split(run_key, N)[i], T)[t]`` -- the key layout of a vmapped per-chain loop such
    as ``jax.vmap(window_adaptation(...).run)(jax.random.split(key, N), positions)``.
    Accepted wherever a kernel takes ``rng_key``."""

    __slots__ = ("run_key", "step")

    def __init__(self, run_key, step: int):
        self.run_key = run_key
        self.step = int(step)


def key_spec(rng_key) -> tuple[int, int, int]:
    """-> (key word 0, key word 1, step_fold) with step_fold = -1 for a plain (step-major) key."""
    if isinstance(rng_key, ChainMajorKey):
        k0, k1 = key_words(rng_key.run_key)
        return k0, k1, rng_key.step
    k0, k1 = key_words(rng_key)
    return k0, k1, -1


def chain_normal(rng_key, n_chains: int, dim: int, *, device, chain_offset: int = 0, child=None):
    """``(n_chains, dim)`` float32 device tensor whose row ``i`` is ``jax.random.normal(k, (dim,))`` with ``k`` chain
    ``i``'s key: ``split(rng_key, .)[chain_offset + i]``, or its step-fold child for a ``ChainMajorKey``.  With
    ``child=0`` or ``child=1``, ``k`` is that child of ``split(k, 2)``; ``child=0`` is the reference's ``key_proposal``
    of an ``rmh`` / ``irmh`` transition.  For user-written proposal generators, which receive the transition's
    ``rng_key`` unchanged (``bjx_rw_noise``)."""
    import torch

    if child not in (None, 0, 1):
        raise ValueError(f"child must be None, 0 or 1, got {child!r}")
    n_chains, dim = int(n_chains), int(dim)
    if n_chains < 0 or dim < 1:
        raise ValueError(f"chain_normal needs n_chains >= 0 and dim >= 1, got {n_chains} and {dim}")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"chain_normal draws on {device}: blackjax_amd runs on ROCm devices only "
                           "(there is no CPU fallback)")
    k0, k1, fold = key_spec(rng_key)
    out = torch.empty((n_chains, dim), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _lib.call("bjx_rw_noise", _lib.current_stream(), k0, k1, int(chain_offset), fold,
                  -1 if child is None else int(child), n_chains, dim, out.data_ptr())
    return out
