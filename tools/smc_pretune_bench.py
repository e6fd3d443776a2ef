#!/usr/bin/env python
"""Secondary benchmark: the three entry points behind pretuning (``bjx_smc_esjd``, ``bjx_smc_pretune_weights``,
``bjx_smc_jitter_gather``), each beside the same arithmetic composed from PyTorch ops on the same device.

HIP-event medians of the time per call in a batch of calls issued back to back, both versions alternating round by
round after a warm-up of every shape, at 65 536 particles with K = D = 256 and with K = 1 (a step size per particle).
The entry points are called on preallocated buffers; the PyTorch versions (fp64 row sums, ``randn`` noise of the whole
``(N, K)`` array, indexing by the ancestors) are what a port without these kernels would run, not bit-equal
restatements.  Every call of a batch works on the next of ``--sets`` copies of its inputs, so that at the default sizes
(64 MiB per array, three sets) no call finds its inputs in the 256 MiB Infinity Cache, left there by an earlier call.
``fraction_of_peak`` is the bytes a call must move (inputs read once, outputs written once) over its time, against
8 TB/s."""
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
ap.add_argument("--particles", type=int, default=65536)
ap.add_argument("--dim", type=int, default=256, help="D of the positions and K of the wide parameter")
ap.add_argument("--sets", type=int, default=3, help="copies of the inputs the calls of a batch rotate through")
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--batch", type=int, default=20, help="calls between the two events of one measurement")
ap.add_argument("--warmup", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda:0")
N, D, S = args.particles, args.dim, args.sets
PEAK = 8e12
ALPHA, SIGMA = 0.05, 0.1
g = torch.Generator(device=dev)
g.manual_seed(0)


def rand(*shape):
    return torch.randn(*shape, device=dev, generator=g)


sets = []
for _ in range(S):
    w = torch.rand(N, device=dev, generator=g)
    sets.append({
        "prev": rand(N, D), "next": rand(N, D), "acc": torch.rand(N, device=dev, generator=g),
        "imm": torch.rand(N, D, device=dev, generator=g) + 0.5, "measure": torch.rand(N, device=dev, generator=g) ** 3,
        "wide": rand(N, D).abs() + 0.1, "scalar": torch.rand(N, device=dev, generator=g) + 0.1,
        "anc": torch.multinomial(w, N, replacement=True).sort().values.int(),
        "out_n": torch.empty(N, device=dev), "out_wide": torch.empty(N, D, device=dev),
    })
sigma = torch.full((1,), SIGMA, device=dev)
key = bjx.random.key_words(bjx.random.key(1))


def esjd_hip(s, imm):
    _lib.call("bjx_smc_esjd", _lib.current_stream(), N, D, s["prev"].data_ptr(), s["next"].data_ptr(),
              s["acc"].data_ptr(), s["imm"].data_ptr() if imm else None, D if imm else 0, s["out_n"].data_ptr())


def esjd_torch(s, imm):
    d = (s["prev"] - s["next"]).double()
    q = d * d / s["imm"].double() if imm else d * d
    m = (q.sum(1) * s["acc"].double()).float()
    return torch.where(torch.isfinite(m) & (m >= 0), m, torch.zeros_like(m))


def weights_hip(s):
    _lib.call("bjx_smc_pretune_weights", _lib.current_stream(), N, ALPHA, s["measure"].data_ptr(),
              s["out_n"].data_ptr())


def weights_torch(s):
    t = ALPHA + s["measure"].double()
    return (t / t.sum()).float()


def jitter_hip(s, wide, log_space):
    p, out = (s["wide"], s["out_wide"]) if wide else (s["scalar"], s["out_n"])
    _lib.call("bjx_smc_jitter_gather", _lib.current_stream(), key[0], key[1], N, N, D if wide else 1, p.data_ptr(),
              s["anc"].data_ptr(), sigma.data_ptr(), 0, 1 if log_space else 0, out.data_ptr())


def jitter_torch(s, wide, log_space):
    p = s["wide"] if wide else s["scalar"]
    z = torch.randn(p.shape, device=dev, generator=g)
    return (p * torch.exp(SIGMA * z) if log_space else p + SIGMA * z)[s["anc"].long()]


mat_b, vec_b = 4 * N * D, 4 * N  # bytes of an (N, D) and of an (N,) array
# name -> (entry point, PyTorch version, bytes a call must move)
cases = {
    "esjd_identity": (lambda s: esjd_hip(s, False), lambda s: esjd_torch(s, False), 2 * mat_b + 2 * vec_b),
    "esjd_per_particle_metric": (lambda s: esjd_hip(s, True), lambda s: esjd_torch(s, True), 3 * mat_b + 2 * vec_b),
    "pretune_weights": (weights_hip, weights_torch, 2 * vec_b),
    "jitter_gather_k256": (lambda s: jitter_hip(s, True, False), lambda s: jitter_torch(s, True, False),
                           2 * mat_b + vec_b),
    "jitter_gather_k256_log": (lambda s: jitter_hip(s, True, True), lambda s: jitter_torch(s, True, True),
                               2 * mat_b + vec_b),
    "jitter_gather_k1": (lambda s: jitter_hip(s, False, False), lambda s: jitter_torch(s, False, False), 3 * vec_b),
    "jitter_gather_k1_log": (lambda s: jitter_hip(s, False, True), lambda s: jitter_torch(s, False, True), 3 * vec_b),
}

for i in range(args.warmup):
    for hip, ref, _ in cases.values():
        hip(sets[i % S])
        ref(sets[i % S])
torch.cuda.synchronize()
marks = {name: {"hip": [], "torch": []} for name in cases}
for _ in range(args.reps):
    for name, (hip, ref, _) in cases.items():
        for which, fn in (("hip", hip), ("torch", ref)):  # a batch of calls back to back between two events
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(args.batch):
                fn(sets[i % S])
            b.record()
            torch.cuda.synchronize()
            marks[name][which].append(a.elapsed_time(b) / args.batch)
median_us = {name: {which: float(np.median(v)) * 1e3 for which, v in m.items()} for name, m in marks.items()}
print(json.dumps({
    "config": {"particles": N, "dim": D, "sets": S, "reps": args.reps, "warmup": args.warmup, "batch": args.batch},
    "median_us": median_us,
    "bytes": {name: c[2] for name, c in cases.items()},
    "fraction_of_peak": {name: cases[name][2] / (median_us[name]["hip"] * 1e-6) / PEAK for name in cases},
}))
