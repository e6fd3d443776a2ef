#!/usr/bin/env python
"""Secondary benchmark: normal_random_walk transitions (blackjax_amd.random_walk) at 65 536 chains x 1 024 dims on a
diagonal Gaussian (sigma_j = 10^(-0.5 + j / (D - 1))), one scale per dimension 2.4 / sqrt(D) sigma_j (acceptance ~ 0.25:
the random walk's optimal scaling).  Run tools/mala_bench.py beside it: k_mala_propose has the same normal per element.

Algorithmic bytes of a transition per (chain, dim) element:
  propose    r q0                  w q1         8 B  (one normal draw per element: VALU-bound, as k_mala_propose)
  callable   r q1                  (w g1)       4 B  value only (8 B as evaluated here: the built-in target writes its
                                                     gradient too, which a gradient-free sampler drops)
  finish     r the chosen row      w q          8 B  (the accept is a per-row scalar; the select is wave-uniform)

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
alg = bjx.normal_random_walk(fn, (2.4 / np.sqrt(D)) * sig)
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
launches = ("bjx_rw_propose", "bjx_target_diag_gaussian", "bjx_rw_finish")
timer = _lib.LaunchTimer(launches, capacity=len(launches) * args.steps)
_lib.set_timer(timer)
for k in keys[args.warmup + args.steps:]:
    state, info = alg.step(k, state)
torch.cuda.synchronize()
_lib.set_timer(None)

bytes_per_elem = {"bjx_rw_propose": 8, "bjx_target_diag_gaussian": 8, "bjx_rw_finish": 8}
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
    "metric": "normal_random_walk transitions/s (no gradient)",
    "value": N / (float(np.median(step_ms)) * 1e-3), "unit": "chain-transitions/s (median transition)",
    "value_mean": N * args.steps / dt,
    "config": {"workload": f"blackjax_amd.normal_random_walk {N} chains x {D} dims, per-dimension sigma, "
                           f"{args.steps} transitions after {args.warmup}"},
    "ms_per_transition": {"median": float(np.median(step_ms)), "min": float(step_ms.min()),
                          "p90": float(np.percentile(step_ms, 90)), "max": float(step_ms.max()),
                          "mean_host_clock": dt / args.steps * 1e3},
    "mean_acceptance": float(acc) / args.steps,
    "bytes_per_element_as_evaluated": total,
    "hbm_floor_us_at_8TBps": total * N * D / 8e12 * 1e6,
    "frac_of_8TBps": total * N * D / (float(np.median(step_ms)) * 1e-3) / 8e12,
    "sum_of_launch_medians_us": sum(v["median_us"] or 0.0 for v in per_launch.values()),
    "per_launch": per_launch,
}
print(json.dumps(out))
