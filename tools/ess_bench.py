#!/usr/bin/env python
"""Secondary benchmark: elliptical slice transitions (blackjax_amd.elliptical_slice) at 65 536 chains x 1 024 dims with a
diagonal Gaussian likelihood (sigma_j = 10^(-0.5 + j / (D - 1))) and a diagonal Gaussian prior (zero mean, variances
sigma_j^2, so the posterior is the likelihood narrowed by sqrt(2)).

Algorithmic bytes per (chain, dim) element:
  begin      r q0                  w nu, q_prop   12 B  (one normal draw per element: VALU-bound, as bjx_mala_propose)
  callable   r q_prop              w g             8 B  (targets.DiagGaussian also writes the gradient nobody reads)
  shrink     r q0, nu              w q_prop       12 B  for a live row; the same, once, with the momentum as the output
                                                        for a row that accepts; one byte per finished row
A transition is begin + R callables + R shrinks, R = the largest sub-iteration count of the batch; every callable sees
all N rows, so the share of callable rows that were already finished is the work live-row compaction would save.

After a warm-up: transitions/s from the median transition (one HIP event per transition boundary; the mean by the
host clock beside it), the sub-iteration histogram of the timed transitions, then the HIP-event time of every launch
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
ap.add_argument("--steps", type=int, default=20, help="timed transitions (at least 10: the per-launch figure is a median)")
ap.add_argument("--warmup", type=int, default=5, help="untimed transitions (code objects, the caching allocator)")
args = ap.parse_args()
if args.steps < 10:
    ap.error("--steps must be at least 10")
dev = torch.device("cuda:0")
N, D = args.chains, args.dim
sig = torch.as_tensor((10.0 ** (-0.5 + 1.0 * np.arange(D) / max(D - 1, 1))).astype(np.float32), device=dev)
fn = bjx.targets.DiagGaussian((1.0 / (sig * sig)).contiguous())
g = torch.Generator(device=dev)
g.manual_seed(0)
q0 = (sig / 2.0 ** 0.5) * torch.randn(N, D, device=dev, generator=g)  # a posterior draw
alg = bjx.elliptical_slice(fn, mean=0.0, cov=(sig * sig).contiguous())
state = alg.init(q0)
keys = bjx.random.split(bjx.random.key(1), 2 * args.steps + args.warmup)
for k in keys[:args.warmup]:
    state, info = alg.step(k, state)
torch.cuda.synchronize()

# end to end, launches not bracketed: one event per transition boundary (median transition) + the host clock (mean)
subiters = []
marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
t0 = time.perf_counter()
marks[0].record()
for i, k in enumerate(keys[args.warmup:args.warmup + args.steps]):
    state, info = alg.step(k, state)
    marks[i + 1].record()
    subiters.append(info.subiter)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
step_ms = np.array([a.elapsed_time(b) for a, b in zip(marks[:-1], marks[1:])])
subiters = torch.stack(subiters).cpu().numpy()  # (steps, N)
hist = np.bincount(subiters.ravel())
rounds = subiters.max(axis=1)
# a chain with s sub-iterations is live in s of its transition's R callables and stale in the other R - s
n_sub = np.arange(hist.size)
rows_called = float(N * rounds.sum())
rows_live = float((hist * n_sub).sum())

# the same number of transitions again with every launch bracketed by HIP events: time per launch
launches = ("bjx_ess_begin", "bjx_target_diag_gaussian", "bjx_ess_shrink")
timer = _lib.LaunchTimer(launches, capacity=len(launches) * args.steps * 16)
_lib.set_timer(timer)
for k in keys[args.warmup + args.steps:]:
    state, info = alg.step(k, state)
torch.cuda.synchronize()
_lib.set_timer(None)

bytes_per_elem = {"bjx_ess_begin": 12, "bjx_target_diag_gaussian": 8, "bjx_ess_shrink": 12}
per_launch = {}
for name in launches:
    ms = np.array(timer.durations_ms(name))
    us = float(np.median(ms)) * 1e3 if ms.size else None
    per_launch[name] = {
        "launches_timed": int(ms.size), "median_us": us,
        "min_us": float(ms.min()) * 1e3 if ms.size else None,
        "max_us": float(ms.max()) * 1e3 if ms.size else None,
        "bytes_per_element_all_rows_live": bytes_per_elem[name],
        "achieved_TBps_if_all_rows_live": bytes_per_elem[name] * N * D / (us * 1e-6) / 1e12 if us else None,
    }
# shrink's time falls with the number of live rows: the first round of a transition against its last
sh = np.array(timer.durations_ms("bjx_ess_shrink"))
out = {
    "metric": "elliptical slice transitions/s (no gradient; one likelihood evaluation per sub-iteration)",
    "value": N / (float(np.median(step_ms)) * 1e-3), "unit": "chain-transitions/s (median transition)",
    "value_mean": N * args.steps / dt,
    "config": {"workload": f"blackjax_amd.elliptical_slice {N} chains x {D} dims, diagonal prior, "
                           f"{args.steps} transitions after {args.warmup}"},
    "ms_per_transition": {"median": float(np.median(step_ms)), "min": float(step_ms.min()),
                          "p90": float(np.percentile(step_ms, 90)), "max": float(step_ms.max()),
                          "mean_host_clock": dt / args.steps * 1e3},
    "subiter": {"mean": rows_live / (N * args.steps), "max": int(n_sub[hist > 0].max()),
                "histogram": {str(int(s)): int(c) for s, c in zip(n_sub, hist) if c},
                "rounds_per_transition": {"mean": float(rounds.mean()), "min": int(rounds.min()),
                                          "max": int(rounds.max())}},
    "callable_rows_already_finished_share": 1.0 - rows_live / rows_called,
    "shrink_us_first_decile_of_launches_by_time": float(np.percentile(sh, 10)) * 1e3 if sh.size else None,
    "shrink_us_last_decile_of_launches_by_time": float(np.percentile(sh, 90)) * 1e3 if sh.size else None,
    "sum_of_launch_medians_us": sum(v["median_us"] or 0.0 for v in per_launch.values()),
    "per_launch": per_launch,
}
print(json.dumps(out))
