#!/usr/bin/env python
"""Secondary benchmark: the SMC arithmetic (blackjax_amd.smc) at 65 536 particles beside one MALA transition at
65 536 x 256, the move it surrounds.

HIP-event medians of: one adaptive temperature solve that bisects (``bjx_smc_ess_solve``: 31 evaluations of the ESS in
one launch of one workgroup), the resampling (prefix scan + ancestor search), the row gather, the reweighting, the
tempered combine, and one ``blackjax_amd.mala`` transition on a diagonal Gaussian of the same shape.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import blackjax_amd as bjx  # noqa: E402
from blackjax_amd import _lib, smc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--particles", type=int, default=65536)
ap.add_argument("--dim", type=int, default=256)
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=10)
args = ap.parse_args()
dev = torch.device("cuda:0")
N, D = args.particles, args.dim
g = torch.Generator(device=dev)
g.manual_seed(0)
x = torch.randn(N, D, device=dev, generator=g)
prior = bjx.targets.DiagGaussian(torch.ones(D, device=dev))
lik = bjx.targets.DiagGaussian(torch.full((D,), 8.0 / D, device=dev))
ll = lik(x)[0]
lam0 = torch.zeros((), device=dev)
keys = bjx.random.split(bjx.random.key(1), args.reps + args.warmup)

launches = ("bjx_smc_ess_solve", "bjx_smc_resample", "bjx_smc_gather", "bjx_smc_reweight", "bjx_smc_temper")
tempered = smc.tempered.TemperedLogDensity(prior, lik)
tempered.set_temperature(torch.full((), 0.3, device=dev))
mala = bjx.mala(prior, 0.05)
state = mala.init(x)


def one_round(k):
    global state
    delta, lam = smc.solver.next_temperature(ll, 0.5, lam0)
    w, inc, _ = smc.base.reweight(ll, lam0, lam)
    anc = smc.resampling.systematic._bjx_trusted(k, w, N)
    smc.base.gather(x, anc)
    tempered(x)
    state, _ = mala.step(k, state)
    return delta


for k in keys[:args.warmup]:
    delta = one_round(k)
torch.cuda.synchronize()
timer = _lib.LaunchTimer(launches, capacity=len(launches) * args.reps)
_lib.set_timer(timer)
marks = []
for k in keys[args.warmup:]:
    one_round(k)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    state, _ = mala.step(k, state)
    b.record()
    marks.append((a, b))
torch.cuda.synchronize()
_lib.set_timer(None)
out = {
    "config": {"particles": N, "dim": D, "reps": args.reps, "warmup": args.warmup, "target_ess": 0.5},
    "delta": float(delta), "bisected": bool(0.0 < float(delta) < 1.0),
    "median_us": {name: float(np.median(timer.durations_ms(name))) * 1e3 for name in launches},
    "mala_transition_median_us": float(np.median([a.elapsed_time(b) for a, b in marks])) * 1e3,
}
print(json.dumps(out))
