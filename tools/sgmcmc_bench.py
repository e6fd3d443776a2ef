#!/usr/bin/env python
"""Secondary benchmark: the stochastic-gradient samplers (blackjax_amd.sgld / sghmc / sgnht) at 65 536 chains x 1 024
dims with an element-wise diagonal-Gaussian "estimator" (g = -q / sigma^2, sigma_j = 10^(-0.5 + j / (D - 1)); the
minibatch is ignored), so that the step kernels dominate, beside one MALA transition in the same process as the
yardstick: bjx_sgld_step moves bjx_mala_propose's bytes and draws the same normal per element.

Algorithmic bytes per (chain, dim) element:
  bjx_sgld_step    r q, g       w q      12 B
  bjx_sghmc_step   r q, p, g    w q, p   20 B  (first step of a transition, momentum drawn: 16; last, position only: 12)
  bjx_sgnht_step   r q, p, g    w q, p   20 B
  bjx_mala_propose r q, g       w q      12 B
  bjx_csgld_step   r q, g       w q      12 B  (+ 12 B per chain: the index and two histogram entries)
  bjx_csgld_update r pdf        w pdf     8 B  per (chain, bin) entry of the (N, M) energy histogram, M = 512

After a warm-up every launch of the timed steps is bracketed by HIP events; the figure per entry point is the median.
bjx_sghmc_step is timed with L = 3: the first / middle / last launch of a transition are told apart by their position in
it.  At the end bjx_sgld_step and bjx_mala_propose alternate on the same three buffers, which takes the neighbouring
launches and the operands' history out of the comparison.  bjx_csgld_step (contour SGLD's position update: sgld's with a
per-chain multiplier on the gradient) then alternates with bjx_sgld_step in the same way, and bjx_csgld_update (its
histogram update) is timed beside a plain PyTorch composition of the same update, bracketed by events as a whole.
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
ap.add_argument("--chains", type=int, default=65536)
ap.add_argument("--dim", type=int, default=1024)
ap.add_argument("--step-size", type=float, default=0.01)
ap.add_argument("--partitions", type=int, default=512, help="bins of csgld's per-chain energy histogram")
ap.add_argument("--steps", type=int, default=60, help="timed steps per sampler (at least 20: the figure is a median)")
ap.add_argument("--warmup", type=int, default=20, help="untimed steps per sampler (code objects, the caching allocator)")
args = ap.parse_args()
if args.steps < 20:
    ap.error("--steps must be at least 20")
dev = torch.device("cuda:0")
N, D, eps = args.chains, args.dim, args.step_size
sig = torch.as_tensor((10.0 ** (-0.5 + 1.0 * np.arange(D) / max(D - 1, 1))).astype(np.float32), device=dev)
neg_inv_var = (-1.0 / (sig * sig)).contiguous()
gen = torch.Generator(device=dev)
gen.manual_seed(0)
q0 = sig * torch.randn(N, D, device=dev, generator=gen)


def estimator(q, minibatch):
    return q * neg_inv_var


def timed(names, step, state, n_timed):
    """Warm up, then bracket every launch of ``names`` over ``n_timed`` steps; -> {name: durations in ms}."""
    keys = bjx.random.split(bjx.random.key(1), args.warmup + n_timed)
    for k in keys[:args.warmup]:
        state = step(k, state)
    torch.cuda.synchronize()
    timer = _lib.LaunchTimer(names, capacity=4 * n_timed)
    _lib.set_timer(timer)
    for k in keys[args.warmup:]:
        state = step(k, state)
    torch.cuda.synchronize()
    _lib.set_timer(None)
    return {n: timer.durations_ms(n) for n in names}


def summary(ms, bytes_per_elem):
    us = float(np.median(ms)) * 1e3
    return {"launches_timed": len(ms), "median_us": us, "min_us": float(np.min(ms)) * 1e3,
            "p90_us": float(np.percentile(ms, 90)) * 1e3, "bytes_per_element": bytes_per_elem,
            "achieved_TBps": bytes_per_elem * N * D / (us * 1e-6) / 1e12}


per_launch = {}

sgld = bjx.sgld(estimator)
ms = timed(("bjx_sgld_step",), lambda k, q: sgld.step(k, q, None, eps), sgld.init(q0), args.steps)
per_launch["bjx_sgld_step"] = summary(ms["bjx_sgld_step"], 12)

sghmc = bjx.sghmc(estimator, 3)
ms = timed(("bjx_sghmc_step",), lambda k, q: sghmc.step(k, q, None, eps), sghmc.init(q0), args.steps)["bjx_sghmc_step"]
for i, (name, b) in enumerate((("first", 16), ("middle", 20), ("last", 12))):
    per_launch[f"bjx_sghmc_step[{name}]"] = summary(ms[i::3], b)

sgnht = bjx.sgnht(estimator)
ms = timed(("bjx_sgnht_step",), lambda k, st: sgnht.step(k, st, None, eps), sgnht.init(q0, bjx.random.key(2)),
           args.steps)
per_launch["bjx_sgnht_step"] = summary(ms["bjx_sgnht_step"], 20)

mala = bjx.mala(bjx.targets.DiagGaussian((1.0 / (sig * sig)).contiguous()), 0.032)
ms = timed(("bjx_mala_propose",), lambda k, st: mala.step(k, st)[0], mala.init(q0), args.steps)
per_launch["bjx_mala_propose"] = summary(ms["bjx_mala_propose"], 12)

# the yardstick again, after everything else: the spread between the two is the run-to-run spread of this process
ms = timed(("bjx_sgld_step",), lambda k, q: sgld.step(k, q, None, eps), sgld.init(q0), args.steps)
per_launch["bjx_sgld_step[again]"] = summary(ms["bjx_sgld_step"], 12)
ms = timed(("bjx_mala_propose",), lambda k, st: mala.step(k, st)[0], mala.init(q0), args.steps)
per_launch["bjx_mala_propose[again]"] = summary(ms["bjx_mala_propose"], 12)

# the two entry points alone, alternating on the SAME three buffers (q, g -> out), so that neither the neighbouring
# launches nor where the operands last lived differ between them: what is left is the kernels' own difference
g0 = estimator(q0, None)
out = torch.empty_like(q0)
k0, k1 = bjx.random.key_words(bjx.random.key(3))
timer = _lib.LaunchTimer(("bjx_sgld_step", "bjx_mala_propose"), capacity=2 * args.steps)
for i in range(args.warmup + args.steps):
    if i == args.warmup:
        torch.cuda.synchronize()
        _lib.set_timer(timer)
    _lib.call("bjx_sgld_step", _lib.current_stream(), k0, k1, 0, i, N, D, eps, None, 1.0, None, q0.data_ptr(),
              g0.data_ptr(), out.data_ptr())
    _lib.call("bjx_mala_propose", _lib.current_stream(), k0, k1, 0, i, N, D, eps, None, q0.data_ptr(), g0.data_ptr(),
              out.data_ptr())
torch.cuda.synchronize()
_lib.set_timer(None)
per_launch["bjx_sgld_step[same buffers]"] = summary(timer.durations_ms("bjx_sgld_step"), 12)
per_launch["bjx_mala_propose[same buffers]"] = summary(timer.durations_ms("bjx_mala_propose"), 12)

# contour SGLD.  bjx_csgld_step against bjx_sgld_step on the same three buffers; the histogram is csgld.init's and the
# indices are spread over [1, M - 1], so that the two histogram entries a chain reads differ from chain to chain
M = args.partitions
cs = bjx.sgmcmc.csgld
pdf0 = cs.init(q0, M).energy_pdf
idx0 = (1 + torch.arange(N, device=dev) % (M - 1)).to(torch.int32)
timer = _lib.LaunchTimer(("bjx_csgld_step", "bjx_sgld_step"), capacity=2 * args.steps)
for i in range(args.warmup + args.steps):
    if i == args.warmup:
        torch.cuda.synchronize()
        _lib.set_timer(timer)
    _lib.call("bjx_csgld_step", _lib.current_stream(), k0, k1, 0, i, N, D, M, 1.0, 10.0, eps, None, 1.0, None,
              q0.data_ptr(), g0.data_ptr(), pdf0.data_ptr(), idx0.data_ptr(), out.data_ptr())
    _lib.call("bjx_sgld_step", _lib.current_stream(), k0, k1, 0, i, N, D, eps, None, 1.0, None, q0.data_ptr(),
              g0.data_ptr(), out.data_ptr())
torch.cuda.synchronize()
_lib.set_timer(None)
per_launch["bjx_csgld_step[same buffers]"] = summary(timer.durations_ms("bjx_csgld_step"), 12)
per_launch["bjx_sgld_step[same buffers, beside csgld]"] = summary(timer.durations_ms("bjx_sgld_step"), 12)

# bjx_csgld_update against the same update composed of PyTorch operations (zeta = 0.75, so that both take a power), on
# the same histogram and the same log-densities; energies spread over all bins
# a power-of-two gap: the bin of an energy does not hang on how a division rounds
GAP, MIN_E, ZETA, EPS_SA = 8.0, 0.0, 0.75, 0.05
ld0 = -(GAP * M) * torch.rand(N, device=dev, generator=gen)


def torch_update(ld, pdf):
    idx = torch.floor((-ld - MIN_E) / GAP + 1.0).clamp(1, M - 1).long()[:, None]
    w = EPS_SA * pdf.gather(1, idx) ** ZETA
    update = (-pdf).scatter_add_(1, idx, torch.ones_like(w))
    return pdf + w * update, idx[:, 0].int()


def summary_rows(ms):
    out_ = summary(ms, 8)
    out_["achieved_TBps"] = 8 * N * M / (out_["median_us"] * 1e-6) / 1e12
    return out_


for _ in range(args.warmup):
    torch_update(ld0, pdf0)
    cs.update_energy_histogram(ld0, pdf0, EPS_SA, zeta=ZETA, energy_gap=GAP, min_energy=MIN_E)
torch.cuda.synchronize()
timer = _lib.LaunchTimer(("bjx_csgld_update",), capacity=args.steps)
_lib.set_timer(timer)
events = []
for _ in range(args.steps):
    cs.update_energy_histogram(ld0, pdf0, EPS_SA, zeta=ZETA, energy_gap=GAP, min_energy=MIN_E)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch_update(ld0, pdf0)
    e1.record()
    events.append((e0, e1))
torch.cuda.synchronize()
_lib.set_timer(None)
per_launch["bjx_csgld_update"] = summary_rows(timer.durations_ms("bjx_csgld_update"))
per_launch["torch composition of csgld_update"] = summary_rows(np.array([a.elapsed_time(b) for a, b in events]))
new_pdf, new_idx = cs.update_energy_histogram(ld0, pdf0, EPS_SA, zeta=ZETA, energy_gap=GAP, min_energy=MIN_E)
t_pdf, t_idx = torch_update(ld0, pdf0)
assert torch.equal(new_idx, t_idx) and torch.allclose(new_pdf, t_pdf, rtol=1e-5, atol=1e-9)

print(json.dumps({
    "metric": "per-launch time of the SGMCMC step kernels (HIP events, median)",
    "config": {"workload": f"blackjax_amd.sgld / sghmc (L = 3) / sgnht, {N} chains x {D} dims, scalar step size {eps}, "
                           f"{args.steps} steps after {args.warmup}; bjx_mala_propose in the same process; csgld with "
                           f"{args.partitions} partitions"},
    "sgld_over_mala_propose": per_launch["bjx_sgld_step"]["median_us"] / per_launch["bjx_mala_propose"]["median_us"],
    "sgld_over_mala_propose_same_buffers": (per_launch["bjx_sgld_step[same buffers]"]["median_us"]
                                            / per_launch["bjx_mala_propose[same buffers]"]["median_us"]),
    "csgld_step_over_sgld_step_same_buffers": (per_launch["bjx_csgld_step[same buffers]"]["median_us"]
                                               / per_launch["bjx_sgld_step[same buffers, beside csgld]"]["median_us"]),
    "csgld_update_over_torch_composition": (per_launch["bjx_csgld_update"]["median_us"]
                                            / per_launch["torch composition of csgld_update"]["median_us"]),
    "per_launch": per_launch,
}))
