#!/usr/bin/env python
"""Secondary benchmark: the entry points behind multinomial / residual resampling, waste-free SMC and the particle
moments, each beside the same arithmetic written with PyTorch ops on the same device.

HIP-event medians of the time per call in a batch of calls issued back to back, both versions alternating in one loop
after a warm-up of every shape: ``bjx_smc_resample_sorted`` (both modes; the host-side permutation of ``residual`` is
formed once, outside the timing), ``bjx_smc_scatter_rows`` (one transition's rows of a waste-free generation) and
``bjx_smc_particle_moments``, each called on preallocated buffers.  The PyTorch versions follow the
reference's formulas in fp64 / fp32 ops (``cumsum``, ``searchsorted``, strided ``copy_``, ``mean`` / ``std``); they
are what a port without these kernels would run, not bit-equal restatements.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import blackjax_amd as bjx  # noqa: E402
from blackjax_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--particles", type=int, default=65536)
ap.add_argument("--dim", type=int, default=256)
ap.add_argument("--p", type=int, default=8, help="waste-free chain length: particles / p chains are stored per call")
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--batch", type=int, default=20, help="calls between the two events of one measurement")
ap.add_argument("--warmup", type=int, default=10)
args = ap.parse_args()
dev = torch.device("cuda:0")
N, D, P = args.particles, args.dim, args.p
M = N // P
g = torch.Generator(device=dev)
g.manual_seed(0)
x = torch.randn(N, D, device=dev, generator=g) * 3.0 + 1.0
w = torch.rand(N, device=dev, generator=g) ** 3
w = (w / w.sum()).contiguous()
moved = torch.randn(M, D, device=dev, generator=g)
out = torch.empty(N, D, device=dev)
keys = bjx.random.split(bjx.random.key(1), args.reps + args.warmup)


def sorted_uniforms_torch(m):
    z = torch.cumsum(-torch.log1p(-torch.rand(m + 1, device=dev, generator=g)).double(), 0)
    return z[:-1] / z[-1]


def multinomial_torch():
    idx = torch.searchsorted(torch.cumsum(w.double(), 0), sorted_uniforms_torch(N))
    return idx.clamp_(max=N - 1).int()


def residual_torch():
    scaled = w.double() * N
    cnt = torch.floor(scaled)
    ccnt, crem = torch.cumsum(cnt, 0), torch.cumsum(scaled - cnt, 0)
    i = torch.arange(N, device=dev, dtype=torch.float64)
    certain = torch.searchsorted(ccnt, i, right=True)
    pos = sorted_uniforms_torch(N)[torch.randperm(N, device=dev, generator=g)]
    drawn = torch.searchsorted(crem, pos * crem[-1])
    return torch.where(i < ccnt[-1], certain, drawn).clamp_(max=N - 1).int()


def scatter_torch():
    out[M + 1::P - 1] = moved


def moments_torch():
    xd = x.double()
    return xd.mean(0).float(), xd.std(0, unbiased=False).float()


torch_versions = {"multinomial": multinomial_torch, "residual": residual_torch, "scatter_rows": scatter_torch,
                  "particle_moments": moments_torch}


lib = _lib.load()
anc = torch.empty(N, dtype=torch.int32, device=dev)
ws_sorted = torch.empty(lib.bjx_smc_resample_sorted_workspace_bytes(N, N) // 8, dtype=torch.int64, device=dev)
ws_mom = torch.empty(lib.bjx_smc_particle_moments_workspace_bytes(N, D) // 8, dtype=torch.float64, device=dev)
mean, std = torch.empty(D, device=dev), torch.empty(D, device=dev)
perm = torch.as_tensor(bjx.random.permutation(bjx.random.key(2), N).astype("int32"), device=dev)


def ours(name, k):
    """The entry point alone, on preallocated buffers (the PyTorch versions allocate their results)."""
    k0, k1 = bjx.random.key_words(k)
    stream = _lib.current_stream()
    if name == "multinomial":
        _lib.call("bjx_smc_resample_sorted", stream, k0, k1, 0, N, N, w.data_ptr(), None, ws_sorted.data_ptr(),
                  anc.data_ptr())
    elif name == "residual":
        _lib.call("bjx_smc_resample_sorted", stream, k0, k1, 1, N, N, w.data_ptr(), perm.data_ptr(),
                  ws_sorted.data_ptr(), anc.data_ptr())
    elif name == "scatter_rows":
        _lib.call("bjx_smc_scatter_rows", stream, M, D, moved.data_ptr(), M + 1, P - 1, out.data_ptr())
    else:
        _lib.call("bjx_smc_particle_moments", stream, N, D, x.data_ptr(), ws_mom.data_ptr(), mean.data_ptr(),
                  std.data_ptr())


for k in keys[:args.warmup]:
    for name, fn in torch_versions.items():
        ours(name, k)
        fn()
torch.cuda.synchronize()
marks = {name: {"hip": [], "torch": []} for name in torch_versions}
for k in keys[args.warmup:]:
    for name, fn in torch_versions.items():
        for which in ("hip", "torch"):  # a batch of calls back to back between two events: time per call in a stream
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.batch):
                ours(name, k) if which == "hip" else fn()
            b.record()
            torch.cuda.synchronize()
            marks[name][which].append(a.elapsed_time(b) / args.batch)
print(json.dumps({
    "config": {"particles": N, "dim": D, "p": P, "reps": args.reps, "warmup": args.warmup, "batch": args.batch},
    "median_us": {name: {which: float(np.median(v)) * 1e3 for which, v in m.items()} for name, m in marks.items()},
}))
