#!/usr/bin/env python
"""Probe: periodic orbital transitions (blackjax_amd.orbital_hmc) at 4 096 chains x period 16 x 256 dims on a diagonal
Gaussian (sigma_j = 10^(-0.5 + j / (D - 1))), scalar step size 0.12 D^(-1/3) / P, shared diagonal metric -- against the
same transition written in plain PyTorch ops in this file (the yardstick: torch's own RNG, softmax and elementwise
kernels around the same HIP target, so the difference is the sampler's part of the transition).

Algorithmic traffic of a transition per chain, in floats (P = period, D = dim):
  open       r q, g of the chosen slot, imm (3 D), weights, directions (2 P)   w q_j, p_half_j (2 P D), steps (P), choice (1)
  callable   r q_j (P D)                                                       w logp_j, g_j (P D + P)
  finish     r p_half_j, g_j (2 P D), imm (D), steps, logp (2 P)               w momentums (P D), weights, directions (2 P), mean, variance (2)

The two versions alternate in one process, round by round; a round is ``--steps`` transitions between two HIP events.
Prints one JSON line: the median and minimum round of each version (us per transition), the HIP-event time of every
launch of the kernels' version (median), and the bytes-moved estimate with the HBM time it implies at 8 TB/s.
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
from blackjax_amd.periodic_orbital import PeriodicOrbitalInfo, PeriodicOrbitalState  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--chains", type=int, default=4096)
ap.add_argument("--period", type=int, default=16)
ap.add_argument("--dim", type=int, default=256)
ap.add_argument("--steps", type=int, default=50, help="transitions per round")
ap.add_argument("--rounds", type=int, default=9, help="rounds per version, alternating")
ap.add_argument("--warmup", type=int, default=20, help="untimed transitions per version")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("orbital_probe needs a GPU: there is nothing to time without one")
dev = torch.device("cuda:0")
N, P, D = args.chains, args.period, args.dim
sig = torch.as_tensor((10.0 ** (-0.5 + 1.0 * np.arange(D) / max(D - 1, 1))).astype(np.float32), device=dev)
fn = bjx.targets.DiagGaussian((1.0 / (sig * sig)).contiguous())
imm = torch.linspace(0.5, 2.0, D, device=dev)
eps = float(0.12 * D ** (-1.0 / 3.0) / P)
gen = torch.Generator(device=dev)
gen.manual_seed(0)
q0 = sig * torch.randn(N, D, device=dev, generator=gen)
alg = bjx.orbital_hmc(fn, eps, imm, P)
rows = torch.arange(N, device=dev)
slots = torch.arange(P, device=dev, dtype=torch.int32)
inf = float("inf")


def torch_step(state):
    """The same transition in plain PyTorch ops (torch's RNG instead of the keyed threefry streams)."""
    q_all, w, dirs, _, g_all = state
    cum = w.cumsum(1)
    r = cum[:, -1] * (1.0 - torch.rand(N, device=dev, generator=gen))
    i = (cum < r[:, None]).sum(1).clamp(max=P - 1)
    q, g, d = q_all[rows, i], g_all[rows, i], dirs[rows, i]
    p = torch.randn(N, D, device=dev, generator=gen) / imm.sqrt()
    s = ((slots[None, :] - d[:, None]).float() * eps)[:, :, None]
    ph = p[:, None, :] + (0.5 * s) * g[:, None, :]
    qn = (q[:, None, :] + s * (imm * ph)).reshape(N * P, D)
    logp, gn = fn(qn)
    pn = ph + (0.5 * s) * gn.view(N, P, D)
    logw = logp.view(N, P) - 0.5 * (imm * pn * pn).sum(-1)
    logw = torch.where(torch.isnan(logw) | (logw == inf), -inf, logw)
    wn = torch.softmax(logw, 1)
    new = PeriodicOrbitalState(qn.view(N, P, D), wn, slots.expand(N, P).contiguous(), logp.view(N, P), gn.view(N, P, D))
    return new, PeriodicOrbitalInfo(pn, wn.mean(1), wn.var(1, unbiased=False))


keys = iter(bjx.random.split(bjx.random.key(1), 2 * args.warmup + (args.rounds + 1) * args.steps))
versions = {"hip": lambda st: alg.step(next(keys), st), "torch_ops": torch_step}
state = {name: alg.init(q0) for name in versions}
for name, step in versions.items():
    for _ in range(args.warmup):
        state[name], info = step(state[name])
torch.cuda.synchronize()

us = {name: [] for name in versions}
for _ in range(args.rounds):
    for name, step in versions.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.steps):
            state[name], info = step(state[name])
        b.record()
        torch.cuda.synchronize()
        us[name].append(a.elapsed_time(b) * 1e3 / args.steps)

# one more round of the kernels' version with every launch bracketed by HIP events: time per launch
launches = ("bjx_orbital_open", "bjx_target_diag_gaussian", "bjx_orbital_finish")
timer = _lib.LaunchTimer(launches, capacity=len(launches) * args.steps)
_lib.set_timer(timer)
for _ in range(args.steps):
    state["hip"], info = versions["hip"](state["hip"])
torch.cuda.synchronize()
_lib.set_timer(None)

floats = {"bjx_orbital_open": (3 * D + 2 * P) + (2 * P * D + P + 1), "bjx_target_diag_gaussian": P * D + (P * D + P),
          "bjx_orbital_finish": (2 * P * D + D + 2 * P) + (P * D + 2 * P + 2)}
per_launch = {}
for name in launches:
    ms = timer.durations_ms(name)
    med = float(np.median(ms)) * 1e3
    per_launch[name] = {"median_us": med, "min_us": float(np.min(ms)) * 1e3, "bytes_per_chain": 4 * floats[name],
                        "achieved_TBps": 4 * floats[name] * N / (med * 1e-6) / 1e12}
total = 4 * sum(floats.values())
out = {
    "metric": "orbital_hmc transition time", "unit": "us per transition (median round)",
    "config": {"workload": f"blackjax_amd.orbital_hmc {N} chains x period {P} x {D} dims, scalar step {eps:.6g}, "
                           f"{args.rounds} alternating rounds of {args.steps} transitions after {args.warmup}"},
    "value": float(np.median(us["hip"])),
    "us_per_transition": {name: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
                          for name, v in us.items()},
    "torch_ops_over_hip": float(np.median(us["torch_ops"]) / np.median(us["hip"])),
    "bytes_per_chain": total, "bytes_per_transition": total * N,
    "hbm_floor_us_at_8TBps": total * N / 8e12 * 1e6,
    "sum_of_launch_medians_us": sum(v["median_us"] for v in per_launch.values()),
    "per_launch": per_launch,
    "final_weights_finite": bool(torch.isfinite(state["hip"].weights).all() and torch.isfinite(state["torch_ops"].weights).all()),
}
print(json.dumps(out))
