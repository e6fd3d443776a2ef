#!/usr/bin/env python
"""Secondary benchmark: Barker-proposal transitions (blackjax_amd.barker) at 65 536 chains x 1 024 dims on a diagonal
Gaussian (sigma_j = 10^(-0.5 + j / (D - 1))), scalar step size 0.38 with the shared diagonal metric sigma^2
(acceptance ~ 0.5 at this shape).  ``--metric per-chain`` hands the same diagonal over as an (N, D) tensor (what a
window adaptation returns), ``--metric none`` passes no metric (choose a smaller step size with it).

Algorithmic bytes of a transition per (chain, dim) element:
  propose    r q0, g0 (, imm)      w q1        12 B  (16 B with a per-chain metric; a normal and a uniform draw and one
                                                      fp64 expit per element: VALU-bound)
  callable   r q1                  w g1         8 B
  finish     r q0, q1, g0, g1      w q, g      24 B  (rows of at most 1 024 floats: nothing is re-read; two fp64
                                                      softplus per element)

Run tools/mala_bench.py beside it on the same machine: the two samplers differ in the propose and finish launches only.

After a warm-up: transitions/s from the median transition (one HIP event per transition boundary; the mean by the
host clock around the region, ended by a device synchronise, beside it), then the HIP-event time of every launch
(median) over as many transitions again.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import blackjax_amd as bjx  # noqa: E402
from blackjax_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--chains", type=int, default=65536)
ap.add_argument("--dim", type=int, default=1024)
ap.add_argument("--step-size", type=float, default=0.38)
ap.add_argument("--metric", choices=("shared", "per-chain", "none"), default="shared")
ap.add_argument("--steps", type=int, default=60, help="timed transitions (at least 20: the per-launch figure is a median)")
ap.add_argument("--warmup", type=int, default=30, help="untimed transitions (code objects, the caching allocator)")
args = ap.parse_args()
if args.steps < 20:
    ap.error("--steps must be at least 20")
dev = torch.device("cuda:0")
N, D = args.chains, args.dim
sig = torch.as_tensor((10.0 ** (-0.5 + 1.0 * np.arange(D) / max(D - 1, 1))).astype(np.float32), device=dev)
fn = bjx.targets.DiagGaussian((1.0 / (sig * sig)).contiguous())
g = torch.Generator(device=dev)
g.manual_seed(0)
q0 = sig * torch.randn(N, D, device=dev, generator=g)
imm = {"shared": lambda: (sig * sig).contiguous(),
       "per-chain": lambda: bjx.metrics.PerChainDiag((sig * sig).expand(N, D).contiguous()),
       "none": lambda: None}[args.metric]()
alg = bjx.barker(fn, args.step_size, imm)
state = alg.init(q0)
keys = bjx.random.split(bjx.random.key(1), 2 * args.steps + args.warmup)
for k in keys[:args.warmup]:
    state, info = alg.step(k, state)
torch.cuda.synchronize()

# end to end, launches not bracketed: one event per transition boundary (median transition) + the host clock (mean)
acc = torch.zeros((), device=dev)
marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
t0 = time.perf_counter()
marks[0].record()
for i, k in enumerate(keys[args.warmup:args.warmup + args.steps]):
    state, info = alg.step(k, state)
    acc += info.acceptance_rate.mean()
    marks[i + 1].record()
torch.cuda.synchronize()
dt = time.perf_counter() - t0
step_ms = np.array([a.elapsed_time(b) for a, b in zip(marks[:-1], marks[1:])])

# the same number of transitions again with every launch bracketed by HIP events: time per launch
launches = ("bjx_barker_propose", "bjx_target_diag_gaussian", "bjx_barker_finish")
timer = _lib.LaunchTimer(launches, capacity=len(launches) * args.steps)
_lib.set_timer(timer)
for k in keys[args.warmup + args.steps:]:
    state, info = alg.step(k, state)
torch.cuda.synchronize()
_lib.set_timer(None)

bytes_per_elem = {"bjx_barker_propose": 16 if args.metric == "per-chain" else 12, "bjx_target_diag_gaussian": 8, "bjx_barker_finish": 24}
per_launch = {}
for name in launches:
    ms = timer.durations_ms(name)
    us = float(np.median(ms)) * 1e3 if ms else None
    per_launch[name] = {
        "launches_timed": len(ms), "median_us": us,
        "min_us": float(np.min(ms)) * 1e3 if ms else None,
        "bytes_per_element": bytes_per_elem[name],
        "achieved_TBps": bytes_per_elem[name] * N * D / (us * 1e-6) / 1e12 if us else None,
        "frac_of_8TBps": bytes_per_elem[name] * N * D / (us * 1e-6) / 8e12 if us else None,
    }
total = sum(bytes_per_elem.values())
out = {
    "metric": "Barker-proposal transitions/s (one gradient per transition)",
    "value": N / (float(np.median(step_ms)) * 1e-3), "unit": "chain-transitions/s (median transition)",
    "value_mean": N * args.steps / dt,
    "config": {"workload": f"blackjax_amd.barker {N} chains x {D} dims, scalar step size {args.step_size}, "
                           f"metric {args.metric}, "
                           f"{args.steps} transitions after {args.warmup}"},
    "ms_per_transition": {"median": float(np.median(step_ms)), "min": float(step_ms.min()),
                          "p90": float(np.percentile(step_ms, 90)), "max": float(step_ms.max()),
                          "mean_host_clock": dt / args.steps * 1e3},
    "mean_acceptance": float(acc) / args.steps,
    "algorithmic_bytes_per_element": total,
    "hbm_floor_us_at_8TBps": total * N * D / 8e12 * 1e6,
    "frac_of_8TBps": total * N * D / (float(np.median(step_ms)) * 1e-3) / 8e12,
    "sum_of_launch_medians_us": sum(v["median_us"] or 0.0 for v in per_launch.values()),
    "per_launch": per_launch,
}
print(json.dumps(out))
