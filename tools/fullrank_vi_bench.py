#!/usr/bin/env python
"""Secondary benchmark: a ``fullrank_vi`` step beside the same step composed from PyTorch ops on the same device.

Both fit a full-covariance Gaussian to the same target, a plain PyTorch function
``z -> (-((z - m) / s)^2 / 2).sum(-1)``, with the package's ``optim.adam``.  The package's step traces that function
into one value-and-gradient kernel and runs ``bjx_vi_fullrank_sample`` and ``bjx_vi_fullrank_grad``; the PyTorch
composition (the unflatten of ``chol_params``, ``randn`` for the whole ``(S, D)`` noise array, a matmul for the draw,
the target under ``torch.autograd``, ``solve_triangular`` for the sticking-the-landing term, a matmul for the outer
product and a gather of its lower triangle) is what a port without these kernels would run, not a bit-equal
restatement.

HIP-event medians of the time per step in a batch of steps issued back to back, the two versions alternating round by
round in one process after a warm-up of every shape, at ``(S, D)`` = (100, 1024), (1 024, 256) and (5, 2 048).  The new
launches are also timed alone, on the step's own buffers: ``sample_launch`` (the triangular product), ``grad_stl`` and
``grad_plain`` (``bjx_vi_fullrank_grad`` with and without the triangular solve; ``solve_launch`` is their difference,
the other launches being the same) and ``outer_launches`` (``grad_plain`` less the mean-field reduction's time at the
same shape, which has the same column sums and scalar but no outer product)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import blackjax_amd as bjx  # noqa: E402
from blackjax_amd import optim  # noqa: E402
from blackjax_amd.vi import fullrank_vi as frvi, meanfield_vi as mfvi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="100x1024,1024x256,5x2048", help="comma-separated SxD")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--batch", type=int, default=10, help="steps between the two events of one measurement")
ap.add_argument("--warmup", type=int, default=20)
args = ap.parse_args()
dev = torch.device("cuda:0")
LR = 0.05
gen = torch.Generator(device=dev)
gen.manual_seed(0)
keys = bjx.random.split(bjx.random.key(1), 4096)


def make_case(S, D):
    m = torch.linspace(-2.0, 2.0, D, device=dev)
    s = torch.exp(torch.linspace(-1.5, 1.0, D, device=dev))

    def fn(z):
        return (-0.5 * ((z - m) / s) ** 2).sum(-1)

    opt = optim.adam(LR)
    hip = {"state": frvi.init(torch.zeros(D, device=dev), opt), "t": 0}

    def hip_step():
        hip["state"], _ = frvi.step(keys[hip["t"] % len(keys)], hip["state"], fn, opt, S)
        hip["t"] += 1

    first = frvi.init(torch.zeros(D, device=dev), opt)
    ref = {"mu": first.mu, "chol": first.chol_params, "opt": first.opt_state}
    rows, cols = torch.tril_indices(D, D, -1, device=dev)
    diag = torch.arange(D, device=dev)

    def torch_step():
        mu, chol = ref["mu"], ref["chol"]
        sigma = torch.exp(chol[:D])
        L = torch.zeros(D, D, device=dev)
        L[rows, cols] = chol[D:]
        L[diag, diag] = sigma
        eps = torch.randn(S, D, device=dev, generator=gen)
        z = (mu + eps @ L.T).requires_grad_(True)
        with torch.enable_grad():
            logp = fn(z)
            (G,) = torch.autograd.grad(logp.sum(), z)
        kl = (-0.5 * eps * eps).sum(1).mean() - chol[:D].sum() - 0.5 * D * np.log(2 * np.pi) - logp.detach().mean()
        u = torch.linalg.solve_triangular(L.T, eps.T, upper=True).T
        w = -u - G
        M = (w.T @ eps) / S
        g_chol = torch.cat([sigma * M[diag, diag], M[rows, cols]])
        updates, ref["opt"] = opt.update((w.mean(0), g_chol), ref["opt"], (mu, chol))
        ref["mu"], ref["chol"] = mu + updates[0], chol + updates[1]
        return kl

    # the new launches alone, on buffers of the step's sizes
    G, logp = torch.randn(S, D, device=dev, generator=gen), torch.randn(S, device=dev, generator=gen)
    rho = torch.zeros(D, device=dev)

    def sample_only():
        frvi.sample(keys[0], hip["state"], S)

    def grad_stl():
        frvi.kl_and_grad(keys[0], hip["state"].mu, hip["state"].chol_params, logp, G, True)

    def grad_plain():
        frvi.kl_and_grad(keys[0], hip["state"].mu, hip["state"].chol_params, logp, G, False)

    def meanfield_grad():
        mfvi.kl_and_grad(keys[0], hip["state"].mu, rho, logp, G, False)

    return {"hip": hip_step, "torch": torch_step, "sample_launch": sample_only, "grad_stl": grad_stl,
            "grad_plain": grad_plain, "meanfield_grad": meanfield_grad}


def timed(fn, batch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / batch


shapes = [tuple(int(v) for v in sh.split("x")) for sh in args.shapes.split(",")]
cases = {sh: make_case(*sh) for sh in shapes}
for fns in cases.values():
    for _ in range(args.warmup):  # past the traced function's first re-check against autograd (its 16th call)
        for fn in fns.values():
            fn()
torch.cuda.synchronize()
marks = {sh: {name: [] for name in fns} for sh, fns in cases.items()}
for _ in range(args.reps):
    for sh, fns in cases.items():
        for name, fn in fns.items():
            marks[sh][name].append(timed(fn, args.batch))
out = {"config": {"reps": args.reps, "batch": args.batch, "warmup": args.warmup}, "shapes": {}}
for (S, D), m in marks.items():
    us = {name: float(np.median(v)) * 1e3 for name, v in m.items()}
    low = {name: float(np.min(v)) * 1e3 for name, v in m.items()}
    out["shapes"][f"{S}x{D}"] = {
        "median_us": us, "min_us": low, "speedup": us["torch"] / us["hip"],
        "solve_launch_us": us["grad_stl"] - us["grad_plain"],
        "outer_launches_us": us["grad_plain"] - us["meanfield_grad"],
        "triangle_fma": S * D * (D + 1) // 2,
    }
print(json.dumps(out))
