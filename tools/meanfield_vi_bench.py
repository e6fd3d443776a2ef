#!/usr/bin/env python
"""Secondary benchmark: a ``meanfield_vi`` step beside the same step composed from PyTorch ops on the same device.

Both fit a diagonal Gaussian to the same target, a plain PyTorch function ``z -> (-((z - m) / s)^2 / 2).sum(-1)``, with
Adam.  The package's step traces that function into one value-and-gradient kernel and runs ``bjx_vi_meanfield_sample``,
``bjx_vi_meanfield_grad`` and ``bjx_optim_adam``; the PyTorch composition (``randn`` for the whole ``(S, D)`` noise array,
``exp``, the target under ``torch.autograd``, ``mean(0)``, Adam written out in tensor ops) is what a port without these
kernels would run, not a bit-equal restatement.

HIP-event medians of the time per step in a batch of steps issued back to back, the two versions alternating round by
round in one process after a warm-up of every shape, at ``(S, D)`` = (100, 65 536) and (1 024, 1 024).  The two launches
that draw the ``S D`` normals (the draw itself, and the reduction that regenerates it) are also timed alone, on the
step's own buffers: ``draw_share`` is their part of the step, and ``*_fraction_of_peak`` the bytes each must move over
its time against 8 TB/s -- a small fraction means the draws, not memory, bound it.  ``step_bytes`` is what a step must
move: z written and read, the gradients written and read, ``16 S D`` bytes and O(S + D) beside."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import blackjax_amd as bjx  # noqa: E402
from blackjax_amd import optim  # noqa: E402
from blackjax_amd.vi import meanfield_vi as mfvi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="100x65536,1024x1024", help="comma-separated SxD")
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--batch", type=int, default=20, help="steps between the two events of one measurement")
ap.add_argument("--warmup", type=int, default=20)
args = ap.parse_args()
dev = torch.device("cuda:0")
PEAK = 8e12
LR, B1, B2, EPS = 0.05, 0.9, 0.999, 1e-8
gen = torch.Generator(device=dev)
gen.manual_seed(0)
keys = bjx.random.split(bjx.random.key(1), 4096)


def make_case(S, D):
    m = torch.linspace(-2.0, 2.0, D, device=dev)
    s = torch.exp(torch.linspace(-1.5, 1.0, D, device=dev))

    def fn(z):
        return (-0.5 * ((z - m) / s) ** 2).sum(-1)

    opt = optim.adam(LR, B1, B2, EPS)
    hip = {"state": mfvi.init(torch.zeros(D, device=dev), opt), "t": 0}

    def hip_step():
        hip["state"], _ = mfvi.step(keys[hip["t"] % len(keys)], hip["state"], fn, opt, S)
        hip["t"] += 1

    ref = {"mu": torch.zeros(D, device=dev), "rho": torch.full((D,), -2.0, device=dev),
           "m": [torch.zeros(D, device=dev), torch.zeros(D, device=dev)],
           "v": [torch.zeros(D, device=dev), torch.zeros(D, device=dev)], "t": 0}

    def torch_step():
        mu, rho = ref["mu"], ref["rho"]
        eps = torch.randn(S, D, device=dev, generator=gen)
        sigma = torch.exp(rho)
        z = (mu + sigma * eps).requires_grad_(True)
        with torch.enable_grad():
            logp = fn(z)
            (G,) = torch.autograd.grad(logp.sum(), z)
        kl = (-0.5 * eps * eps).sum(1).mean() - rho.sum() - 0.5 * D * np.log(2 * np.pi) - logp.detach().mean()
        grads = ((-eps / sigma - G).mean(0), (-eps * eps - G * sigma * eps).mean(0))
        ref["t"] += 1
        c1, c2 = 1.0 - B1 ** ref["t"], 1.0 - B2 ** ref["t"]
        new = []
        for i, (p, g) in enumerate(zip((mu, rho), grads)):
            ref["m"][i] = (1.0 - B1) * g + B1 * ref["m"][i]
            ref["v"][i] = (1.0 - B2) * (g * g) + B2 * ref["v"][i]
            new.append(p - LR * (ref["m"][i] / c1) / (torch.sqrt(ref["v"][i] / c2) + EPS))
        ref["mu"], ref["rho"] = new
        return kl

    # the two launches that draw, alone, on buffers of the step's sizes
    G, logp = torch.randn(S, D, device=dev, generator=gen), torch.randn(S, device=dev, generator=gen)

    def sample_only():
        mfvi.sample(keys[0], hip["state"], S)

    def grad_only():
        mfvi.kl_and_grad(keys[0], hip["state"].mu, hip["state"].rho, logp, G)

    return {"hip": hip_step, "torch": torch_step, "sample_launch": sample_only, "grad_launches": grad_only}


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
    sample_bytes, grad_bytes = 4 * S * D + 8 * D, 4 * S * D + 4 * S + 12 * D
    out["shapes"][f"{S}x{D}"] = {
        "median_us": us, "min_us": low, "speedup": us["torch"] / us["hip"],
        "step_bytes": 16 * S * D, "step_fraction_of_peak": 16 * S * D / (us["hip"] * 1e-6) / PEAK,
        "draw_share": (us["sample_launch"] + us["grad_launches"]) / us["hip"],
        "sample_fraction_of_peak": sample_bytes / (us["sample_launch"] * 1e-6) / PEAK,
        "grad_fraction_of_peak": grad_bytes / (us["grad_launches"] * 1e-6) / PEAK,
    }
print(json.dumps(out))
