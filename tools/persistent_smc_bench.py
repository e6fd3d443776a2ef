#!/usr/bin/env python
"""Probe: the persistent-sampling arithmetic of blackjax_amd.smc.persistent_sampling at N = 4 096 particles per
iteration, at iteration i = 8 and i = 64 (P = i N = 32 768 and 262 144 persistent particles) -- against the same
arithmetic composed from PyTorch ops on the device in this file (the yardstick).

Two sequences are timed at each shape:
  weights   bjx_smc_persistent_denominator + bjx_smc_persistent_weights (den, W, log_Z)
            torch: logsumexp over the (i, P) matrix lambda_s ll_j - logZ_s, then logsumexp over P and exp
  solve     bjx_smc_persistent_ess_solve (31 evaluations of f, the bracket on the device; den given)
            torch: the same 31-evaluation bisection with 0-d tensors and torch.where, no host read
The torch versions run in fp32 (what a user would write) and in fp64 (the precision of the kernels' sums).

The versions alternate in one process, round by round; a round is ``--reps`` calls between two HIP events.  Prints one
JSON line: the median, minimum and maximum round of each version in us per call, and the ratio of medians.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blackjax_amd import _lib  # noqa: E402
from blackjax_amd.smc import persistent_sampling as ps  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--particles", type=int, default=4096)
ap.add_argument("--iterations", type=int, nargs="+", default=[8, 64])
ap.add_argument("--reps", type=int, default=20, help="calls per round")
ap.add_argument("--rounds", type=int, default=9, help="rounds per version, alternating")
ap.add_argument("--warmup", type=int, default=5, help="untimed calls per version")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("persistent_smc_bench needs a GPU: there is nothing to time without one")
dev = torch.device("cuda:0")
N = args.particles
HALVINGS = 30


def make_case(i):
    """Slots 0 .. i live: log-likelihoods -8 z^2, a schedule rising from 0 to 0.6, log_Z_s = log E exp(lambda_s ll)."""
    gen = torch.Generator(device=dev)
    gen.manual_seed(i)
    pll = -8.0 * torch.randn(i + 1, N, device=dev, generator=gen) ** 2
    sched = (0.6 * (torch.arange(i + 1, device=dev) / i) ** 2).float()
    plz = (-0.5 * torch.log1p(16.0 * sched.double())).float()
    return pll.contiguous(), plz.contiguous(), sched.contiguous()


def torch_den(pll, plz, sched, i, dtype):
    ll = pll.view(-1)[: i * N].to(dtype)
    lam = sched[:i].to(dtype)
    a = torch.where(lam[:, None] == 0, torch.zeros((), dtype=dtype, device=dev), lam[:, None] * ll[None, :])
    return ll, torch.logsumexp(a - plz[:i].to(dtype)[:, None], 0) - math.log(i)


def torch_weights(pll, plz, sched, i, dtype):
    ll, den = torch_den(pll, plz, sched, i, dtype)
    lw = sched[i].to(dtype) * ll - den
    lse = torch.logsumexp(lw, 0)
    return torch.exp(lw - lse).float(), (lse - math.log(i * N)).float()


def torch_solve(ll, den, lam_old, log_target):
    def f(d):
        lw = (lam_old + d) * ll - den
        return 2.0 * torch.logsumexp(lw, 0) - torch.logsumexp(2.0 * lw, 0) - log_target

    max_delta = 1.0 - lam_old
    full = f(max_delta) >= 0
    lo, hi = torch.zeros_like(max_delta), max_delta
    for _ in range(HALVINGS):
        mid = 0.5 * (lo + hi)
        up = f(mid) >= 0
        lo, hi = torch.where(up, mid, lo), torch.where(up, hi, mid)
    return torch.where(full, max_delta, lo)


def time_versions(versions):
    for fn in versions.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name in versions}
    for _ in range(args.rounds):
        for name, fn in versions.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            us[name].append(a.elapsed_time(b) * 1e3 / args.reps)
    out = {name: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
           for name, v in us.items()}
    for name in versions:
        if name != "hip":
            out[name + "_over_hip"] = out[name]["median"] / out["hip"]["median"]
    return out


results = {}
for i in args.iterations:
    pll, plz, sched = make_case(i)
    P = i * N
    den = ps._denominator(pll, plz, sched, i)
    ws = ps._workspace(P, dev)
    delta = torch.empty((), device=dev)
    lam_new = torch.empty((), device=dev)
    lam_old = sched[i - 1].clone()
    # a target between the ESS at the two ends of the interval, so that the solve bisects (one host read, untimed)
    ll64, den64 = pll.view(-1)[:P].double(), den.double()
    ends = []
    for lam in (lam_old.double(), 1.0):
        lw64 = lam * ll64 - den64
        ends.append(float(torch.exp(2.0 * torch.logsumexp(lw64, 0) - torch.logsumexp(2.0 * lw64, 0))))
    target = math.sqrt(ends[0] * ends[1])

    def hip_solve():
        _lib.call("bjx_smc_persistent_ess_solve", _lib.current_stream(), P, pll.data_ptr(), den.data_ptr(), target,
                  lam_old.data_ptr(), ws.data_ptr(), delta.data_ptr(), lam_new.data_ptr())

    weights = {"hip": lambda: ps._weigh(pll, plz, sched, i, i, False, True)}
    solve = {"hip": hip_solve}
    for label, dtype in (("torch_ops_fp32", torch.float32), ("torch_ops_fp64", torch.float64)):
        weights[label] = lambda dtype=dtype: torch_weights(pll, plz, sched, i, dtype)
        ll_t, den_t = pll.view(-1)[:P].to(dtype), den.to(dtype)
        solve[label] = lambda ll_t=ll_t, den_t=den_t, dtype=dtype: torch_solve(ll_t, den_t, lam_old.to(dtype),
                                                                               math.log(target))
    # the two versions agree before they are timed
    w_h, z_h = weights["hip"]()[1:]
    w_t, z_t = weights["torch_ops_fp64"]()
    hip_solve()
    d_t = solve["torch_ops_fp64"]()
    results[f"i={i}"] = {
        "P": P,
        "weights_us": time_versions(weights),
        "solve_us": time_versions(solve),
        "max_weight_difference_x_P": float((w_h - w_t).abs().max() * P), "log_Z": [float(z_h), float(z_t)],
        "ess_at_the_ends": ends, "target": target, "delta": [float(delta), float(d_t)],
        "bisects": bool(0.0 < float(delta) < 1.0 - float(lam_old)),
    }
print(json.dumps({
    "metric": "persistent-sampling weights and temperature solve", "unit": "us per call (median round)",
    "config": {"workload": f"N = {N}, iterations {args.iterations}, {args.rounds} "
                           f"alternating rounds of {args.reps} calls after {args.warmup}"},
    "results": results,
}))
