#!/usr/bin/env python
"""Secondary benchmark: the launches of a blackjax_amd.mgrad_gaussian transition, with the MALA kernels timed in the
same process on the same buffers as yardsticks.  Nothing is gated on these numbers.

Diagonal prior, 65 536 chains x 1 024 dims (U = I: the eigenbasis rows are the position and gradient rows):
  bjx_mgrad_propose r U_x, U_grad_x              w t        12 B   one normal per element
  bjx_mala_propose  r q, g                       w q        12 B   one normal per element (yardstick)
  bjx_mgrad_finish  r 4 eigenbasis rows          w 2 rows   24 B   resident form (D <= 1 024)
  bjx_mala_finish   r q0, q1, g0, g1             w q, g     24 B   resident form (yardstick)
Dense prior, 8 192 chains x 512 dims:
  bjx_mgrad_propose, bjx_mala_propose                       12 B
  bjx_dense_matmul(t, U_t) = y ; bjx_dense_matmul_bt(y, U, U_t) = U_y ; bjx_dense_matmul_bt(g_y, U, U_t) = U_grad_y
                                                             8 B + 2 D flop per element each
  bjx_mgrad_finish  r 4 eigenbasis rows, the selected position and gradient   w 4 rows   40 B
  bjx_mala_finish                                           24 B

The likelihood is a diagonal Gaussian evaluated eagerly once to fill the buffers (it is not timed).  After a warm-up
the entry points alternate on the same buffers, every launch bracketed by HIP events; the figure is the median.
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
ap.add_argument("--steps", type=int, default=40, help="timed launches per entry point (at least 20: a median)")
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--delta", type=float, default=0.05)
args = ap.parse_args()
if args.steps < 20:
    ap.error("--steps must be at least 20")
dev = torch.device("cuda:0")
k0, k1 = bjx.random.key_words(bjx.random.key(3))
stream = _lib.current_stream()


def summary(ms, bytes_per_elem, n_elem):
    us = float(np.median(ms)) * 1e3
    return {"launches_timed": len(ms), "median_us": us, "min_us": float(np.min(ms)) * 1e3,
            "p90_us": float(np.percentile(ms, 90)) * 1e3, "bytes_per_element": bytes_per_elem,
            "achieved_TBps": bytes_per_elem * n_elem / (us * 1e-6) / 1e12}


def alternate(launches):
    """``launches``: {name: callable(step_index)}; all run once per round, in order -> {name: durations in ms}."""
    timer = _lib.LaunchTimer(tuple(launches), capacity=len(launches) * args.steps)
    for i in range(args.warmup + args.steps):
        if i == args.warmup:
            torch.cuda.synchronize()
            _lib.set_timer(timer)
        for fn in launches.values():
            fn(i)
    torch.cuda.synchronize()
    _lib.set_timer(None)
    return {n: timer.durations_ms(n) for n in launches}


def case(N, D, dense):
    sig = torch.as_tensor((10.0 ** (-0.5 + 1.0 * np.arange(D) / max(D - 1, 1))).astype(np.float32), device=dev)
    inv_var = (1.0 / (sig * sig)).contiguous()
    gamma = (sig * sig).contiguous()  # the prior's spectrum: as wide as the likelihood's
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    delta = args.delta
    if dense:
        U = torch.linalg.qr(torch.randn(D, D, generator=gen, device=dev, dtype=torch.float64))[0].float().contiguous()
        U_t = U.t().contiguous()
    x = sig * torch.randn(N, D, device=dev, generator=gen)

    def lik(q):
        g = -(q * inv_var)
        return 0.5 * (q * g).sum(-1), g

    def rot(a):
        out = torch.empty_like(a)
        _lib.call("bjx_dense_matmul_bt", stream, N, D, a.data_ptr(), U.data_ptr(), U_t.data_ptr(), out.data_ptr())
        return out

    logp_x, g_x = lik(x)
    ux, ugx = (rot(x), rot(g_x)) if dense else (x, g_x)
    t = torch.empty_like(x)

    def propose(i):
        _lib.call("bjx_mgrad_propose", stream, k0, k1, 0, i, N, D, delta, None, gamma.data_ptr(), ux.data_ptr(),
                  ugx.data_ptr(), t.data_ptr())

    propose(-1)
    y = torch.empty_like(x) if dense else t
    if dense:
        _lib.call("bjx_dense_matmul", stream, N, D, t.data_ptr(), U_t.data_ptr(), y.data_ptr())
    logp_y, g_y = lik(y)
    g_y = g_y.contiguous()
    uy, ugy = (rot(y), rot(g_y)) if dense else (y, g_y)
    outs = [torch.empty_like(x) for _ in range(4 if dense else 2)]
    logp_o, rate = torch.empty_like(logp_x), torch.empty_like(logp_x)
    acc = torch.empty(N, dtype=torch.bool, device=dev)
    pos = ([x.data_ptr(), g_x.data_ptr(), y.data_ptr(), g_y.data_ptr(), outs[2].data_ptr(), outs[3].data_ptr()]
           if dense else [None] * 6)
    scratch = torch.empty_like(x)

    def finish(i):
        _lib.call("bjx_mgrad_finish", stream, k0, k1, 0, i, N, D, delta, None, gamma.data_ptr(), pos[0],
                  logp_x.data_ptr(), pos[1], ux.data_ptr(), ugx.data_ptr(), pos[2], logp_y.data_ptr(), pos[3],
                  uy.data_ptr(), ugy.data_ptr(), pos[4], logp_o.data_ptr(), pos[5], outs[0].data_ptr(),
                  outs[1].data_ptr(), rate.data_ptr(), acc.data_ptr())

    def mala_propose(i):  # the same two operands and the same output buffer as bjx_mgrad_propose
        _lib.call("bjx_mala_propose", stream, k0, k1, 0, i, N, D, delta, None, ux.data_ptr(), ugx.data_ptr(),
                  scratch.data_ptr())

    def mala_finish(i):  # the same four operand rows and two output rows as bjx_mgrad_finish
        _lib.call("bjx_mala_finish", stream, k0, k1, 0, i, N, D, delta, None, ux.data_ptr(), logp_x.data_ptr(),
                  ugx.data_ptr(), uy.data_ptr(), logp_y.data_ptr(), ugy.data_ptr(), outs[0].data_ptr(),
                  logp_o.data_ptr(), outs[1].data_ptr(), rate.data_ptr(), acc.data_ptr())

    def propose_scratch(i):
        _lib.call("bjx_mgrad_propose", stream, k0, k1, 0, i, N, D, delta, None, gamma.data_ptr(), ux.data_ptr(),
                  ugx.data_ptr(), scratch.data_ptr())

    launches = {"bjx_mgrad_propose": propose_scratch, "bjx_mala_propose": mala_propose, "bjx_mgrad_finish": finish,
                "bjx_mala_finish": mala_finish}
    finish(-1)
    accept_share = float(acc.float().mean())
    ms = alternate(launches)
    n = N * D
    res = {"bjx_mgrad_propose": summary(ms["bjx_mgrad_propose"], 12, n),
           "bjx_mala_propose": summary(ms["bjx_mala_propose"], 12, n),
           "bjx_mgrad_finish": summary(ms["bjx_mgrad_finish"], 40 if dense else 24, n),
           "bjx_mala_finish": summary(ms["bjx_mala_finish"], 24, n)}
    if dense:
        gemm_out = torch.empty_like(x)
        ms = alternate({"bjx_dense_matmul": lambda i: _lib.call(
            "bjx_dense_matmul", stream, N, D, t.data_ptr(), U_t.data_ptr(), gemm_out.data_ptr())})
        res["bjx_dense_matmul(t, U_t)"] = summary(ms["bjx_dense_matmul"], 8, n)
        ms = alternate({"bjx_dense_matmul_bt": lambda i: _lib.call(
            "bjx_dense_matmul_bt", stream, N, D, (y if i % 2 == 0 else g_y).data_ptr(), U.data_ptr(), U_t.data_ptr(),
            gemm_out.data_ptr())})["bjx_dense_matmul_bt"]
        res["bjx_dense_matmul_bt(y, U, U_t)"] = summary(ms[(args.warmup % 2)::2], 8, n)
        res["bjx_dense_matmul_bt(g_y, U, U_t)"] = summary(ms[1 - (args.warmup % 2)::2], 8, n)
        for k in list(res):
            if "matmul" in k:
                res[k]["achieved_TFLOPs"] = 2.0 * D * n / (res[k]["median_us"] * 1e-6) / 1e12
    ratios = {"mgrad_propose_over_mala_propose": res["bjx_mgrad_propose"]["median_us"] / res["bjx_mala_propose"]["median_us"],
              "mgrad_finish_over_mala_finish": res["bjx_mgrad_finish"]["median_us"] / res["bjx_mala_finish"]["median_us"]}
    return {"chains": N, "dim": D, "prior": "dense" if dense else "diagonal", "delta": delta,
            "accepted_share": accept_share, **ratios, "per_launch": res}


print(json.dumps({
    "metric": "per-launch time of the mgrad_gaussian kernels (HIP events, median), MALA kernels on the same buffers",
    "config": {"steps": args.steps, "warmup": args.warmup},
    "diagonal": case(65536, 1024, False),
    "dense": case(8192, 512, True),
}))
