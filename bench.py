#!/usr/bin/env python
"""Headline benchmark: chain-leapfrog-steps/sec of batched diagonal-mass HMC on MI355X.

``--config c2`` (default; BASELINE.json configs[1], SURVEY.md section 8d "C2"): 65 536 chains x
1 024-dim diagonal Gaussian (sigma_i = 10^(-1+2i/(D-1))), inverse mass = sigma^2, eps = 0.25,
L = 50 leapfrog steps per transition, fp32.  A "step" is one HMC transition of every chain
(momentum draw, L leapfrogs each followed by the log-density callable, Metropolis accept).
``--config c4`` (configs[3]): ``window_adaptation(hmc, L = 50)`` on the 4 096-dim ill-conditioned
Gaussian, 32 768 chains PER GPU (262 144 on 8 GPUs) with per-chain step size and per-chain inverse
mass matrix; a "step" is one warm-up step (transition + dual averaging + Welford) of every chain.
Chains shard over GPUs with no data-path collective (weak scaling); per-chain keys come from the
global chain index (``chain_offset = rank * chains_per_gpu``).

Launching: ``python bench.py --gpus N`` with N > 1 and no torchrun environment re-executes itself
under ``python -m torch.distributed.run --nproc-per-node N`` (one rank per GPU over RCCL) and
REFUSES to run when fewer than N GPUs are visible -- it never reports fewer ranks than asked for.
Under torchrun (RANK / WORLD_SIZE set) ``--gpus`` must equal WORLD_SIZE.  Rank 0 prints ONE JSON
line with ``n_gpus`` = the ranks RCCL saw, every rank's device and time, and the max over ranks.

Scheduling of a C2 transition (``--chain-block``): chains are independent, so the engine may run
a transition block by block over chains -- same kernels, same results bit for bit.  A block whose
q, p, g fit the 256 MiB Infinity Cache (16 384 chains at D = 1 024) re-reads its state from the
cache across the L steps.  The default autotunes in the warm-up (two untimed transitions per
candidate: cache blocks with plain launches, cache blocks with the inner loop as a HIP graph when
the host's launch rate is close to the GPU's pace, all chains per launch), the fastest candidate
is THE timed region; the others are measured afterwards for the roofline object.

A plain run (``python bench.py --gpus 1 --steps K --warmup W``) sets up, warms up (the scheduling autotune
included), times the K steps and prints the result line; ``--dump-outputs DIR`` adds what the timed call returned
in its last step as ``DIR/<name>.npy`` (see ``write_outputs``).  Every other measurement or check of this file
(launch-timed rooflines, the user-callable and ESS regions, parity against the oracle, the CPU baseline, the
jax.random pin, the C3 / C5 / C4 sub-objects of the default run, the extra regions of ``--config c3/c4/c5``)
runs only with ``--full``.

JSON extras (``--full``; contract in the task statement):
  roofline      dominant kernel = fused kick+drift leapfrog, ALGORITHMIC bytes per launch
                (20 B x D x chains per launch: read p,g,q; write p,q) / mean launch duration measured
                with HIP events on the launch stream inside a timed region.  ``frac`` is the
                HBM-STREAMING measurement (all chains per launch: every launch moves 1.3 GB through
                HBM); ``cache_assisted_frac`` is the same kernel on Infinity-Cache blocks, where
                part of the traffic never reaches HBM -- it can exceed what HBM alone delivers and
                is reported under that name only.  ``traffic`` comes from the committed PMC summary
                (``traffic_source`` says so; it is not measured in this run).
  torch_callable_mode   the same workload with the user log-density as a plain PyTorch function handed to hmc(...) as is
                (the path north_star names): by default traced on its first call into one generated value-and-gradient
                kernel; torch_autograd_mode = the same function kept on eager autograd (blackjax_amd.no_trace).
  stdout        ONE compact JSON line (<= 6 KB: headline keys, roofline, cpu_baseline, parity, per-config value /
                roofline / parity counts); the FULL object goes to stderr and gpurun_out/bench_full_latest.json
                ($BJX_BENCH_FULL); --full-line prints the full object on stdout instead.
  ess / ess_nonresonant   min-ESS per second on the contract parameters (eps*L = 12.5 ~ 4 pi: a
                resonant trajectory length, every transition returns near its start) and on
                eps = 0.21 (same cost per transition, non-resonant).
  parity        BASELINE.md section 3's parity columns, per config (top level = C2; c3_nuts.parity, c5_dense.parity): one
                more transition AFTER the timed regions, engine over all chains vs the oracle on a spread subset --
                accept_mismatches, max_abs_dpos, max_abs_dmean, max_abs_dvar, chains_checked.
  cpu_baseline  BlackJAX on JAX-CPU when ``import jax, blackjax`` works on this box ("reference"),
                else the oracle's C/OpenMP port ("port"); bounded sample, rank 0, N = 1 only.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def sigma_ladder(D, lo=-1.0, hi=1.0):
    return (10.0 ** (lo + (hi - lo) * np.arange(D) / (D - 1))).astype(np.float32)


def load_tool(name):
    """tools/<name>.py loaded BY PATH: ``tools/`` is a plain directory, and a regular top-level
    ``tools`` package elsewhere on sys.path would shadow a ``from tools import ...``."""
    import importlib.util

    spec = importlib.util.spec_from_file_location(f"_bjx_tool_{name}", os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rng_pin_check(dev):
    """The jax.random self-check (does something only where ``import jax`` works); never raises."""
    try:
        return load_tool("rng_pin").check(dev)
    except Exception as e:
        return f"unavailable: tools/rng_pin.py could not be loaded or run ({type(e).__name__}: {e})"


# ------------------------------------------------------------------------------------ CPU baseline
def cpu_baseline_port(D, L, eps, target_seconds):
    """The oracle's C port (all host cores) on a bounded sample of the same workload."""
    from oracle import cport, prng

    sig = sigma_ladder(D)
    imm = (sig * sig).astype(np.float32)
    inv_var = (np.float32(1.0) / imm).astype(np.float32)
    threads = cport.num_threads()
    n = 8 * threads
    rng = np.random.default_rng(0)
    n_big = 2048 * threads
    q = (sig * rng.standard_normal((n_big, D))).astype(np.float32)
    g = (-(q * inv_var)).astype(np.float32)
    logp = (0.5 * np.sum(q.astype(np.float64) * g, axis=-1)).astype(np.float32)
    cport.hmc_diag_gaussian_step(prng.key(0), q[:n], logp[:n], g[:n], eps, imm, inv_var, L)  # warm
    keys = prng.split(prng.key(1), 1000)
    done = 0
    t0 = time.perf_counter()
    while done < 2 or (time.perf_counter() - t0 < target_seconds and done < len(keys)):
        cport.hmc_diag_gaussian_step(keys[done], q, logp, g, eps, imm, inv_var, L)
        done += 1
    dt = time.perf_counter() - t0
    return {
        "value": n_big * L * done / dt, "unit": "chain-leapfrog-steps/s", "cores": threads,
        "kind": "port",
        "sample": f"{n_big} chains x {D} dims, L={L}, {done} transitions ({dt:.1f} s) -- C/OpenMP "
                  "port of the oracle (a CPU restatement of BlackJAX's arithmetic, NOT JAX)",
    }


def cpu_baseline_jax(D, L, eps, target_seconds):
    """BlackJAX itself on JAX-CPU: jit(scan(vmap(kernel.step))) -- only when both import here."""
    os.environ.setdefault("JAX_PLATFORMS", "cpu")
    import jax  # ImportError -> the caller falls back to the port and reports why
    import jax.numpy as jnp
    import blackjax

    sig = jnp.asarray(sigma_ladder(D))
    imm = sig * sig
    inv_var = 1.0 / imm

    def logdensity(q):
        return -0.5 * jnp.sum(q * q * inv_var)

    alg = blackjax.hmc(logdensity, eps, imm, L)
    cores = os.cpu_count() or 1
    n, T = 64 * cores, 4
    q0 = sig * jax.random.normal(jax.random.key(1), (n, D), dtype=jnp.float32)
    states = jax.vmap(alg.init)(q0)

    @jax.jit
    def run(states, key):
        def body(st, k):
            st, info = jax.vmap(alg.step)(jax.random.split(k, n), st)
            return st, info.acceptance_rate.mean()

        return jax.lax.scan(body, states, jax.random.split(key, T))

    states, _ = run(states, jax.random.key(0))
    jax.block_until_ready(states)
    done = 0
    t0 = time.perf_counter()
    while done < 1 or time.perf_counter() - t0 < target_seconds:
        states, acc = run(states, jax.random.key(2 + done))
        jax.block_until_ready(states)
        done += 1
    dt = time.perf_counter() - t0
    return {
        "value": n * L * T * done / dt, "unit": "chain-leapfrog-steps/s", "cores": cores,
        "kind": "reference",
        "sample": f"blackjax {getattr(blackjax, '__version__', '?')} on jax {jax.__version__} (CPU), "
                  f"jit(scan(vmap(step))): {n} chains x {D} dims, L={L}, {T * done} transitions "
                  f"({dt:.1f} s), mean acceptance {float(acc[-1]):.3f}",
    }


def cpu_baseline(D, L, eps, target_seconds=15.0):
    """First try the real thing, then the port; say which and why."""
    try:
        return cpu_baseline_jax(D, L, eps, target_seconds)
    except Exception as e:  # ImportError on a box without jax/blackjax wheels, or any runtime failure
        out = cpu_baseline_port(D, L, eps, target_seconds)
        out["jax_baseline"] = f"unavailable on this box ({type(e).__name__}: {e})"
        return out


# ------------------------------------------------------------------------------------ launching
# ------------------------------------------------------------------------------------ parity (checker leg)
# BASELINE.md section 3 asks for "accept-index mismatches vs oracle, max |d mean|, |d var|" NEXT TO the throughput.
# After the timed regions (never inside them) one more transition of the benchmarked state is taken by the engine
# over all chains and recomputed for a spread subset of chains by the oracle (oracle/: the CPU restatement of the
# reference's arithmetic, test infrastructure -- here the CHECKER, never the thing measured).  The subset's
# per-chain keys are the rows of split(key, N_total) at the chains' global indices, so the subset run IS those chains.
def _spread_chains(N, blocks, n_total, seed):
    """First / last chains, both sides of every boundary of each block size, random fill up to n_total chains."""
    idx = {0, 1, 2, 3, 63, 64, N - 2, N - 1}
    for b in blocks:
        if b and b < N:
            for m in range(b, N, b):
                idx.update((m - 1, m))
    idx = {i for i in idx if 0 <= i < N}
    rng = np.random.default_rng(seed)
    pool = np.setdiff1d(np.arange(N), np.fromiter(idx, dtype=np.int64))
    if n_total > len(idx):
        idx.update(int(i) for i in rng.choice(pool, min(n_total - len(idx), len(pool)), replace=False))
    return np.array(sorted(idx), dtype=np.int64)


def _moment_deltas(a, b):
    """max over dimensions of |mean_a - mean_b| and |var_a - var_b| across the checked chains (fp64 moments)."""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    return (float(np.max(np.abs(a64.mean(0) - b64.mean(0)))), float(np.max(np.abs(a64.var(0) - b64.var(0)))))


def parity_c2(bjx, dev, rank, state, target, imm, inv_var, N, D, L, eps, sched):
    """One more C2 transition from the benchmarked state: engine (all chains, the headline's scheduling) vs the
    oracle's C port on >= 512 chains spread over every chain block."""
    from oracle import cport, prng

    t0 = time.perf_counter()
    cb, gr, ns = sched
    idx = _spread_chains(N, (cb, 4096), 512, seed=17)
    t = torch.as_tensor(idx, device=dev)
    q = state.position[t].cpu().numpy().copy()
    lp = state.logdensity[t].cpu().numpy().copy()
    g = state.logdensity_grad[t].cpu().numpy().copy()
    alg = bjx.hmc(target, eps, imm, L, chain_offset=rank * N, chain_block=cb, use_graph=gr, streams=ns)
    key = bjx.random.key(424242)
    st1, info = alg.step(key, state)
    acc_o, ia_o, idv_o = cport.hmc_diag_gaussian_step_pc(
        prng.split_at(np.asarray(key), idx + rank * N), q, lp, g, eps,
        imm.cpu().numpy(), inv_var.cpu().numpy(), L)
    pos_g = st1.position[t].cpu().numpy()
    dmean, dvar = _moment_deltas(pos_g, q)
    ia_g = info.is_accepted[t].cpu().numpy().astype(bool)
    return {"checked_against": "oracle/c (C port of the oracle, bit-identical to oracle/hmc.py: tests/test_oracle_c.py)",
            "transition": "one transition after the timed region, from the benchmarked state, fresh key",
            "chains_checked": int(len(idx)), "chain_blocks_covered": int(len(np.unique(idx // cb))),
            "chain_blocks_total": int((N + cb - 1) // cb),
            "accept_mismatches": int(np.sum(ia_g != ia_o)),
            "divergence_mismatches": int(np.sum(info.is_divergent[t].cpu().numpy().astype(bool) != idv_o)),
            "max_abs_dacceptance_rate": float(np.max(np.abs(info.acceptance_rate[t].cpu().numpy() - acc_o))),
            "max_abs_dpos": float(np.max(np.abs(pos_g - q))),
            "max_abs_dgrad": float(np.max(np.abs(st1.logdensity_grad[t].cpu().numpy() - g))),
            "max_abs_dmean": dmean, "max_abs_dvar": dvar,
            "rejected_among_checked": int(np.sum(~ia_o)), "seconds": time.perf_counter() - t0}


def parity_c5(bjx, dev, rank, alg, state, N, D, L, eps, rho):
    """One more C5 transition: engine (MFMA GEMM chain) vs oracle/hmc.py in its f32-chain mode (the stated k order of
    v_mfma_f32_32x32x2_f32, oracle/fp.py) on >= 256 chains, at least one in every 128-row GEMM tile.  The oracle runs
    with the engine's fp32 factor L^-T (so the GEMM chain is compared bit for bit); the factor itself is compared
    with the oracle's own fp64 Cholesky / triangular inverse and the difference reported."""
    from oracle import hmc as ohmc
    from oracle import prng
    from oracle import targets as otargets

    t0 = time.perf_counter()
    f32 = np.float32
    rng = np.random.default_rng(23)
    idx = np.unique(np.concatenate([_spread_chains(N, (4096,), 128, seed=29),
                                    np.arange(0, N, 128) + rng.integers(0, 128, (N + 127) // 128)]))
    idx = idx[idx < N]
    t = torch.as_tensor(idx, device=dev)
    cov = otargets.ar1_covariance(rho, D)
    fn_o = otargets.ar1_gaussian(rho, D)
    m = bjx.metrics.default_metric(torch.as_tensor(cov, device=dev), N, D, dev)
    mass_sqrt = np.ascontiguousarray(m.mass_sqrt_t.cpu().numpy().T)
    own = ohmc.default_metric(cov).mass_matrix_sqrt
    factor_abs = float(np.max(np.abs(mass_sqrt - own)))  # (relative to the largest entry: the factor is banded, most entries ~ 0)
    metric = ohmc.default_metric(cov, dense_accum="f32chain", mass_matrix_sqrt=mass_sqrt)
    st_s = ohmc.HMCState(state.position[t].cpu().numpy().copy(), state.logdensity[t].cpu().numpy().copy(),
                         state.logdensity_grad[t].cpu().numpy().copy())
    key = bjx.random.key(515151)
    st1, info = alg.step(key, state)
    key_np = np.asarray(key)
    st_s, info_s = ohmc.kernel(None, st_s, fn_o, f32(eps), cov, L, metric=metric,
                               chain_keys_override=prng.split_at(key_np, idx + rank * N))
    pos_g = st1.position[t].cpu().numpy()
    dmean, dvar = _moment_deltas(pos_g, st_s.position)
    return {"checked_against": "oracle/hmc.py, dense_accum='f32chain' (fp32 fma chain in the MFMA's k order), engine's fp32 factor",
            "transition": "one transition after the timed region, from the benchmarked state, fresh key",
            "chains_checked": int(len(idx)), "gemm_tiles_covered": int(len(np.unique(idx // 128))),
            "gemm_tiles_total": int((N + 127) // 128),
            "accept_mismatches": int(np.sum(info.is_accepted[t].cpu().numpy().astype(bool) != info_s.is_accepted)),
            "divergence_mismatches": int(np.sum(info.is_divergent[t].cpu().numpy().astype(bool) != info_s.is_divergent)),
            "max_abs_dacceptance_rate": float(np.max(np.abs(info.acceptance_rate[t].cpu().numpy() - info_s.acceptance_rate))),
            "max_abs_dmomentum_draw": float(np.max(np.abs(info.momentum[t].cpu().numpy() - info_s.momentum))),
            "max_abs_dpos": float(np.max(np.abs(pos_g - st_s.position))),
            "max_abs_dmean": dmean, "max_abs_dvar": dvar,
            "factor_max_abs_diff_vs_oracle_own_cholesky": factor_abs, "factor_max_abs_entry": float(np.max(np.abs(own))),
            "rejected_among_checked": int(np.sum(~info_s.is_accepted)), "seconds": time.perf_counter() - t0}


def parity_c3(bjx, dev, rank, alg, state, N, D, eps, max_depth):
    """One more lockstep NUTS transition: engine (all chains) vs oracle/nuts.py on 120+ chains spread over the batch
    plus the chains that built the deepest trees of this transition (chosen from the engine's record; the oracle
    recomputes them from scratch)."""
    from oracle import hmc as ohmc
    from oracle import nuts as onuts
    from oracle import prng
    from oracle import targets as otargets

    t0 = time.perf_counter()
    f32 = np.float32
    key = bjx.random.key(313131)
    st1, info = alg.step(key, state)
    deepest = torch.topk(info.num_integration_steps, 8).indices.cpu().numpy()
    idx = np.unique(np.concatenate([_spread_chains(N, (8192,), 120, seed=31), deepest]))
    t = torch.as_tensor(idx, device=dev)
    st_s = ohmc.HMCState(state.position[t].cpu().numpy().copy(), state.logdensity[t].cpu().numpy().copy(),
                         state.logdensity_grad[t].cpu().numpy().copy())
    key_np = np.asarray(key)
    st_s, info_s = onuts.kernel(None, st_s, otargets.neal_funnel(), f32(eps), np.ones(D, f32), max_depth,
                                chain_keys_override=prng.split_at(key_np, idx + rank * N))
    pos_g = st1.position[t].cpu().numpy()
    dmean, dvar = _moment_deltas(pos_g, st_s.position)
    mism = {name: int(np.sum(getattr(info, name)[t].cpu().numpy() != getattr(info_s, name)))
            for name in ("num_integration_steps", "num_trajectory_expansions", "is_turning", "is_divergent")}
    return {"checked_against": "oracle/nuts.py (NumPy restatement of nuts.py / trajectory.py / termination.py)",
            "transition": "one lockstep transition after the timed regions, from the benchmarked state, fresh key",
            "chains_checked": int(len(idx)),
            "accept_mismatches": int(np.sum(np.any(pos_g != st_s.position, axis=1) & (np.max(np.abs(pos_g - st_s.position), axis=1) > 1e-5))),
            "accept_note": "NUTS has no accept bit: a chain counts as a mismatch when its selected proposal differs from the oracle's by more than 1e-5 anywhere",
            "tree_size_mismatches": mism["num_integration_steps"], "tree_depth_mismatches": mism["num_trajectory_expansions"],
            "turning_flag_mismatches": mism["is_turning"], "divergence_mismatches": mism["is_divergent"],
            "max_abs_dpos": float(np.max(np.abs(pos_g - st_s.position))),
            "frac_position_elements_not_bit_equal": float(np.mean(pos_g != st_s.position)),
            "max_abs_dacceptance_rate": float(np.max(np.abs(info.acceptance_rate[t].cpu().numpy() - info_s.acceptance_rate))),
            "max_abs_dmean": dmean, "max_abs_dvar": dvar,
            "largest_tree_checked": int(np.max(info_s.num_integration_steps)),
            "tree_depths_checked": sorted(set(int(d) for d in info_s.num_trajectory_expansions)),
            "seconds": time.perf_counter() - t0}


def _try_parity(fn, *a):
    try:
        return fn(*a)
    except Exception as e:  # the parity block is a reported extra; it must never fail the throughput line
        return {"error": repr(e)[:400]}


def _r(x, sig=6):
    """Numbers of the compact line: 6 significant digits."""
    if isinstance(x, bool) or x is None or isinstance(x, (int, str)):
        return x
    if isinstance(x, float):
        if x == x and abs(x) < 2.0 ** 53 and x.is_integer():
            return int(x)
        return float(f"{x:.{sig}g}") if x == x and abs(x) != float("inf") else None
    if isinstance(x, (list, tuple)):
        return [_r(v, sig) for v in x]
    if isinstance(x, dict):
        return {k: _r(v, sig) for k, v in x.items()}
    return x


def _pick(d, *keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d}


_PARITY_KEYS = ("chains_checked", "accept_mismatches", "divergence_mismatches", "tree_size_mismatches",
                "tree_depth_mismatches", "turning_flag_mismatches", "max_abs_dpos", "max_abs_dmean", "max_abs_dvar",
                "max_abs_dacceptance_rate", "largest_tree_checked", "chain_blocks_covered", "chain_blocks_total",
                "gemm_tiles_covered", "gemm_tiles_total", "error")
_ROOF_KEYS = ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_us", "launches_timed",
              "algorithmic_bytes_per_chain_leapfrog",
              "algorithmic_bytes_per_launch", "algorithmic_flops_per_launch", "chains_per_launch", "mode",
              "cache_assisted_frac", "traffic_over_algorithmic", "frac_at_measured_bytes",
              "busy_phase_tick_frac_measured", "full_ensemble_tick_us", "traffic_build")


def compact_line(out, full_path):
    """The ONE stdout line of the contract, <= 6 KB (the driver keeps an 8 KB tail of stdout: round 5's 25 KB line lost
    C5's, C3's and the parity blocks' values): headline keys + config + roofline + cpu_baseline + parity + for each of
    C3 / C4 / C5 {value, ms_per_step, roofline, parity counts} + the non-degenerate ESS/s.  The FULL object goes to
    stderr and to `full_path`."""
    c = _pick(out, "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "mean_acceptance", "end_to_end_frac_of_28B_roofline", "ranks",
              "backend", "per_rank_ms_per_step", "devices_distinct", "n_gpus_note")
    if isinstance(out.get("roofline"), dict):
        c["roofline"] = _pick(out["roofline"], *_ROOF_KEYS)
        ts = out["roofline"].get("traffic_source")
        if ts:
            c["roofline"]["traffic_source"] = ts[:160]
    if "cpu_baseline" in out:
        c["cpu_baseline"] = dict(out["cpu_baseline"])
        if isinstance(c["cpu_baseline"].get("sample"), str):
            c["cpu_baseline"]["sample"] = c["cpu_baseline"]["sample"][:180]
        if isinstance(c["cpu_baseline"].get("jax_baseline"), str):
            c["cpu_baseline"]["jax_baseline"] = c["cpu_baseline"]["jax_baseline"][:80]
    if isinstance(out.get("parity"), dict):
        c["parity"] = _pick(out["parity"], *_PARITY_KEYS)
    if isinstance(out.get("ess"), dict):
        c["ess_per_sec_contract_params"] = out["ess"].get("min_ess_per_sec_all_chains")
        c["ess_note"] = "contract eps*L = 12.5 ~ 4*pi: degenerate; quote ess_nonresonant"
    if isinstance(out.get("ess_nonresonant"), dict):
        c["ess_nonresonant"] = _pick(out["ess_nonresonant"], "min_ess_per_sec_all_chains", "min_ess_subset", "subset_chains",
                                     "draws_per_chain", "eps", "leapfrogs", "ms_per_step", "mean_acceptance")
    for name in ("torch_callable_mode", "torch_autograd_mode", "torch_elementwise_mode", "torch_compile_mode"):
        if isinstance(out.get(name), dict):
            c[name] = _pick(out[name], "value", "ms_per_step", "frac_of_28B_roofline", "path", "error")
    for name in ("c5_dense", "c3_nuts", "c4_shard"):
        sub = out.get(name)
        if not isinstance(sub, dict):
            continue
        o = _pick(sub, "value", "unit", "steps", "ms_per_step", "mean_acceptance", "error", "end_to_end_frac_of_32B_roofline",
                  "mean_leapfrogs_per_chain_transition", "utilisation")
        if isinstance(sub.get("config"), dict) and "workload" in sub["config"]:
            o["workload"] = sub["config"]["workload"][:140]
        if isinstance(sub.get("roofline"), dict):
            o["roofline"] = _pick(sub["roofline"], *_ROOF_KEYS)
        if isinstance(sub.get("parity"), dict):
            o["parity"] = _pick(sub["parity"], *_PARITY_KEYS)
        for k in ("free_running_T400", "lockstep_step"):
            if isinstance(sub.get(k), dict):
                o[k] = _pick(sub[k], "value", "ms_per_transition", "frac_of_52B_roofline")
        c[name] = o
    for k in ("rng_pin", "oracle_pin"):
        if isinstance(out.get(k), str):
            c[k] = out[k][:120]
    c["full_record"] = full_path
    c = _r(c)
    line = json.dumps(c, separators=(",", ":"))
    # hard bound: drop the least important keys until the line fits
    for k in ("oracle_pin", "rng_pin", "torch_compile_mode", "torch_elementwise_mode", "per_rank_ms_per_step", "ess_note",
              "torch_autograd_mode"):
        if len(line) <= 6000:
            break
        c.pop(k, None)
        line = json.dumps(c, separators=(",", ":"))
    return line


def write_full_record(out):
    """The full object: stderr (one line, prefixed) + a file under gpurun_out/ (merged back by gpurun) -- copy the ones to
    be judged into profiles/."""
    text = json.dumps(out)
    sys.stderr.write("bench.py FULL RECORD: " + text + "\n")
    sys.stderr.flush()
    path = os.environ.get("BJX_BENCH_FULL", os.path.join("gpurun_out", "bench_full_latest.json"))
    try:
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as fh:
            fh.write(text + "\n")
    except OSError as e:
        print(f"bench.py: could not write {path}: {e!r}", file=sys.stderr)
        path = "stderr"
    return path


DUMP_MAX_BYTES = 64 * 10 ** 6
DUMP_SAMPLED_BYTES = 48 << 20  # what the chain-sampled arrays may take together
DUMP_WHOLE_BYTES = 1 << 20  # arrays up to this size are written whole


def _dump_leaves(x, name):
    """(name, tensor or number) for every array of a returned structure: NamedTuple fields, dict keys and tuple
    indices joined with '.'; None and other objects are skipped."""
    if isinstance(x, torch.Tensor):
        yield name, x
    elif isinstance(x, (bool, int, float)):
        yield name, torch.tensor(float(x), dtype=torch.float64)
    elif hasattr(x, "_fields"):
        for f in x._fields:
            yield from _dump_leaves(getattr(x, f), f"{name}.{f}" if name else f)
    elif isinstance(x, dict):
        for k in sorted(x):
            yield from _dump_leaves(x[k], f"{name}.{k}" if name else str(k))
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            yield from _dump_leaves(v, f"{name}.{i}" if name else str(i))


def write_outputs(out_dir, returned, n_chains):
    """``--dump-outputs``: every array of ``returned`` (what the timed call handed its caller in the last timed step)
    as ``out_dir/<name>.npy`` -- float32 stays float32; float64, integer and boolean arrays are written as float64.
    Arrays larger than 1 MiB with a chain axis keep a fixed sample of chains (seed 0, drawn from the chain count alone,
    so two builds write the same chains; listed in ``chain_sample.npy``), sized so that they take at most 48 MiB
    together.  The whole dump is at most 64 MB."""
    leaves = []
    for name, t in _dump_leaves(returned, ""):
        t = t.detach()
        t = t.float() if t.dtype in (torch.float16, torch.bfloat16, torch.float32) else t.double()
        axis = next((a for a, s in enumerate(t.shape) if s == n_chains), None)
        leaves.append((name, t, axis if t.numel() * t.element_size() > DUMP_WHOLE_BYTES else None))
    per_chain = sum(t.numel() * t.element_size() // n_chains for _, t, a in leaves if a is not None)
    k = min(n_chains, max(1, DUMP_SAMPLED_BYTES // max(per_chain, 1)))
    arrays = {}
    if k < n_chains:
        idx = np.sort(np.random.default_rng(0).permutation(n_chains)[:k])
        arrays["chain_sample"] = idx.astype(np.float64)
    for name, t, axis in leaves:
        if axis is not None and k < n_chains:
            t = t.index_select(axis, torch.as_tensor(idx, device=t.device))
        arrays[name] = t.cpu().numpy()
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_MAX_BYTES:
        raise SystemExit(f"bench.py --dump-outputs: {total} bytes exceed {DUMP_MAX_BYTES} "
                         f"({', '.join(f'{n} {a.shape}' for n, a in arrays.items())})")
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)



def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def spawn_ranks(args):
    """``--gpus N`` without a torchrun environment: re-execute under torch.distributed.run, one
    rank per GPU.  Fails loudly when the box cannot give N ranks their own GPU."""
    n = args.gpus
    backend = os.environ.get("BJX_BENCH_BACKEND", "nccl")
    if not args.selftest_control_flow and backend == "nccl":
        have = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if have < n:
            sys.exit(f"bench.py --gpus {n}: only {have} GPU(s) visible on this box -- refusing to run "
                     f"(a {n}-GPU figure needs {n} GPUs; nothing is reported instead of n_gpus < {n})")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)]
    cmd += sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    sys.exit(subprocess.call(cmd, env=env))


class Ctx:
    """Rank / device / collectives of this process."""

    def __init__(self, args):
        import torch.distributed as dist

        self.dist = dist
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        self.cpu_only = bool(args.selftest_control_flow)
        if self.world != args.gpus:
            raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={self.world}: launch with "
                             f"--nproc-per-node {args.gpus} (or drop the torchrun environment and let "
                             "bench.py spawn its ranks)")
        self.backend = None
        # BJX_BENCH_FORCE_PG=1: initialise the process group and run every collective of this file even
        # with ONE rank (tests/test_rccl_gpu.py: RCCL loaded and used on a one-GPU box)
        self.collective = self.world > 1 or os.environ.get("BJX_BENCH_FORCE_PG", "0") == "1"
        if self.collective:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", str(_free_port()))
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
            # One rank per GPU over RCCL (backend "nccl").  BJX_BENCH_BACKEND=gloo exists only so the
            # multi-rank control flow can be exercised on a single-GPU or GPU-less box.
            self.backend = "gloo" if self.cpu_only else os.environ.get("BJX_BENCH_BACKEND", "nccl")
        if self.cpu_only:
            self.dev = torch.device("cpu")
        else:
            assert torch.cuda.is_available(), "bench.py needs a GPU (blackjax_amd has no CPU fallback)"
            n_dev = torch.cuda.device_count()
            if self.backend == "nccl" and n_dev < self.world:
                raise SystemExit(f"bench.py: {self.world} ranks but {n_dev} GPU(s) visible")
            self.local_rank %= max(n_dev, 1)
            self.dev = torch.device("cuda", self.local_rank)
            torch.cuda.set_device(self.dev)
        if self.collective:
            if self.backend == "nccl":
                dist.init_process_group("nccl", device_id=self.dev)
            else:
                dist.init_process_group(self.backend)

    def barrier(self):
        if self.collective:
            self.dist.barrier()

    def sync(self):
        if not self.cpu_only:
            torch.cuda.synchronize()

    def max_over_ranks(self, dt):
        """-> (max, [per-rank values])"""
        if not self.collective:
            return dt, [dt]
        t = torch.tensor([dt], device=self.coll_dev, dtype=torch.float64)
        out = [torch.empty_like(t) for _ in range(self.world)]
        self.dist.all_gather(out, t)
        per = [float(o.item()) for o in out]
        return max(per), per

    def ranks_seen(self):
        me = {"rank": self.rank, "local_rank": self.local_rank, "device": str(self.dev),
              "name": "cpu" if self.cpu_only else torch.cuda.get_device_name(self.dev),
              "pid": os.getpid()}
        if not self.collective:
            return [me]
        out = [None] * self.world
        self.dist.all_gather_object(out, me)
        return out

    @property
    def coll_dev(self):
        """Device the collectives run on: the GPU under RCCL; gloo gathers go through host memory."""
        return self.dev if self.backend == "nccl" else torch.device("cpu")

    def gather_rows(self, x):
        if not self.collective:
            return x
        x = x.to(self.coll_dev).contiguous()
        out = [torch.empty_like(x) for _ in range(self.world)]
        self.dist.all_gather(out, x)
        return torch.cat(out, 0)

    def finish(self):
        if self.collective:
            self.dist.destroy_process_group()


def timed_region(ctx, step_fn, steps):
    """The contract's timing: barrier + synchronize, EXACTLY ``steps`` calls of ``step_fn(i)``,
    synchronize + barrier; returns (max over ranks of the wall time, per-rank times, this rank's
    host enqueue time)."""
    ctx.barrier()
    ctx.sync()
    t0 = time.perf_counter()
    for i in range(steps):
        step_fn(i)
    t_enq = time.perf_counter() - t0
    ctx.sync()
    ctx.barrier()
    dt = time.perf_counter() - t0
    mx, per = ctx.max_over_ranks(dt)
    return mx, per, t_enq


def selftest_control_flow(args, ctx, emit):
    """CPU-only exercise of this file's multi-rank control flow (spawn, rendezvous, barriers,
    max-over-ranks timing, gather, one JSON line from rank 0) with a sleep in place of the GPU step.
    NOT a measurement: ``value`` is null and the metric says so."""
    for _ in range(args.warmup):
        time.sleep(0.001)
    dt, per, _ = timed_region(ctx, lambda i: time.sleep(0.002 * (1 + ctx.rank)), args.steps)
    rows = ctx.gather_rows(torch.full((2, 3), float(ctx.rank)))
    seen = ctx.ranks_seen()
    if ctx.rank == 0:
        emit({
            "metric": "control-flow self-test (no GPU work; NOT a measurement)", "value": None,
            "unit": None, "n_gpus": ctx.world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "per_rank_ms_per_step": [p / args.steps * 1e3 for p in per],
            "ranks_seen": seen, "backend": ctx.backend, "gathered_rows": list(rows.shape),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None})


# ------------------------------------------------------------------------------------ C2
def bench_c2(args, ctx):
    import blackjax_amd as bjx
    from blackjax_amd import _lib
    from blackjax_amd.hmc import auto_chain_block

    dev, world, rank = ctx.dev, ctx.world, ctx.rank
    N, D, L = args.chains or 65536, args.dim or 1024, args.leapfrogs
    blk_auto = min(auto_chain_block(N, D), N)
    sig = torch.as_tensor(sigma_ladder(D), device=dev)
    imm = (sig * sig).contiguous()
    inv_var = (1.0 / imm).contiguous()
    target = bjx.targets.DiagGaussian(inv_var)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234 + rank)
    q_init = sig * torch.randn(N, D, device=dev, generator=gen)
    keys = bjx.random.split(bjx.random.key(0), args.warmup + args.steps)
    n_sub = min(1024, N)
    timed_kernel = "bjx_leapfrog_diag"

    def measure(chain_block, use_graph, collect_draws, steps=None, fn=None, eps=None, timing=True, streams=1,
                dump=False):
        """W warm-up + K timed transitions in one scheduling mode.  The warm-up runs EXACTLY the
        timed loop's body (bookkeeping torch ops and launch-timer events included) plus one priming
        pass: on a fresh box the first use of any kernel pages its code object in from disk, which
        must not land in the timed region.  ``dump``: the region whose last step --dump-outputs writes."""
        steps = args.steps if steps is None else steps
        alg = bjx.hmc(target if fn is None else fn, args.eps if eps is None else eps, imm, L,
                      chain_offset=rank * N, chain_block=chain_block, use_graph=use_graph,
                      streams=streams)
        state = alg.init(q_init)
        launches = L * ((N + chain_block - 1) // chain_block)
        # Sampling rate of the HIP-event brackets.  A bracket costs host time and drains the
        # queue around the launch; at ~50 us launches, bracketing every 4th one slowed the whole
        # timed region by 13 %, so short launches are sampled sparsely.
        every = args.time_every or (16 if launches >= 100 else 1)
        # no events inside a graph; the launch timings feed the roofline, a --full figure
        timing = timing and args.full and not args.no_launch_timing and not use_graph
        cap = (launches // every + 1) * (max(steps, args.warmup + 1))
        warm_timer = _lib.LaunchTimer([timed_kernel], every, cap) if timing else None
        _lib.set_timer(warm_timer)
        warm_acc = torch.zeros((), device=dev)
        prime_key = bjx.random.key(12345)
        for t in range(-1, args.warmup):
            state, info = alg.step(prime_key if t < 0 else keys[t], state)
            warm_acc += info.acceptance_rate.mean()
            _ = state.position[:n_sub].clone()
        _lib.set_timer(None)
        if warm_timer is not None:
            warm_timer.durations_ms(timed_kernel)  # first elapsed_time() call warms that path too
        torch.cuda.synchronize()

        timer = None
        if timing and rank == 0:
            timer = _lib.LaunchTimer([timed_kernel], every, cap)
            torch.cuda.synchronize()
            _lib.set_timer(timer)
        acc_sum = torch.zeros((), device=dev)
        draws = []  # retained draws of a fixed chain subset for ESS/sec (4 MiB per step at C2)
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        for ev in marks:
            ev.record()  # HIP events are created at the first record(): do that outside the region
        box = {"state": state}

        def one(i):
            if i == 0:
                marks[0].record()
            st, info = alg.step(keys[(args.warmup + i) % len(keys)], box["state"])
            box["state"], box["info"] = st, info
            acc_sum.add_(info.acceptance_rate.mean())
            if collect_draws:
                draws.append(st.position[:n_sub].clone())
            marks[i + 1].record()

        dt, per, t_enq = timed_region(ctx, one, steps)
        _lib.set_timer(None)
        if dump and args.dump_outputs and rank == 0:
            write_outputs(args.dump_outputs, {"state": box["state"], "info": box["info"]}, N)
        # host cost of issuing ONE transition into an empty queue (outside the timed region): the
        # in-region enqueue time below also contains the time launch calls block once the host has
        # run ahead as far as the queue allows, so it tracks the GPU time, not the host's work
        t_issue = None
        if args.full:
            torch.cuda.synchronize()
            t_i = time.perf_counter()
            alg.step(prime_key, box["state"])
            t_issue = (time.perf_counter() - t_i) * 1e3
            torch.cuda.synchronize()
        res = {"chain_block": chain_block, "hip_graph": bool(use_graph), "streams": streams, "dt": dt,
               "per_rank_dt": per,
               "steps": steps, "ms_per_step": dt / steps * 1e3,
               "value": world * N * L * steps / dt,
               "host_enqueue_ms_per_step": t_enq / max(steps, 1) * 1e3,
               "host_issue_ms_unthrottled": t_issue,
               "gpu_ms_of_each_step": [round(a.elapsed_time(b), 3) for a, b in zip(marks, marks[1:])],
               "mean_acceptance": float(acc_sum.item()) / max(steps, 1), "draws": draws,
               "state": box["state"], "launch": None,
               "timed": bool(timing)}  # rank independent (the events themselves are rank 0's only)
        if timer is not None:
            d_ms = timer.durations_ms(timed_kernel)
            avg_s = float(np.mean(d_ms)) * 1e-3
            alg_bytes = 20.0 * D * min(chain_block, N)  # read p,g,q ; write p,q (imm (D,) is shared and cached)
            res["launch"] = {"chains_per_launch": min(chain_block, N), "avg_launch_us": avg_s * 1e6,
                             "algorithmic_bytes_per_launch": alg_bytes,
                             "achieved": alg_bytes / avg_s / 1e9, "launches_timed": len(d_ms),
                             "timed_every": every}
        return res

    # ---- scheduling autotune (untimed, part of the warm-up)
    # candidates: (chains per block, inner loop as a HIP graph, blocks in flight on their own streams)
    candidates = [(blk_auto, False, 1)]
    if args.chain_block >= 0:
        candidates = [(min(args.chain_block or N, N), bool(args.use_graph), max(1, args.streams))]
    elif blk_auto < N:
        candidates += [(blk_auto, True, 1), (max(blk_auto // 2, 1024), False, 2), (N, False, 1)]
        if world > 1:
            # no HIP-graph candidate under a process group: a capture that fails on one rank only (the
            # RCCL watchdog thread polls events while another thread captures) would desynchronise the
            # ranks' barriers; the graph mode has not won the autotune on any single-GPU box either
            candidates = [c for c in candidates if not c[1]]
    tuning = {}
    if len(candidates) > 1:
        for cb, gr, ns_ in candidates:
            try:
                alg_t = bjx.hmc(target, args.eps, imm, L, chain_offset=rank * N, chain_block=cb, use_graph=gr,
                                streams=ns_)
                st_t = alg_t.init(q_init)
                # 3 priming transitions (graph recording, allocator) + 5 timed ones: with 2 + 2 the
                # candidates within 3 % of each other were ranked by noise (NOTEBOOK.md section 5)
                for kk in bjx.random.split(bjx.random.key(777), 3):
                    st_t, _ = alg_t.step(kk, st_t)
                torch.cuda.synchronize()
                t_t = time.perf_counter()
                for kk in bjx.random.split(bjx.random.key(778), 5):
                    st_t, _ = alg_t.step(kk, st_t)
                torch.cuda.synchronize()
                tuning[(cb, gr, ns_)] = (time.perf_counter() - t_t) / 5 * 1e3
                del alg_t, st_t
            except Exception as e:  # a mode that cannot run here is simply not a candidate
                tuning[(cb, gr, ns_)] = float("inf")
                if rank == 0:
                    print(f"bench.py: candidate chain_block={cb} hip_graph={gr} streams={ns_} failed: {e!r}",
                          file=sys.stderr)
        if ctx.collective:  # every rank must benchmark the same mode
            t = torch.tensor([tuning[c] for c in candidates], device=ctx.coll_dev, dtype=torch.float64)
            ctx.dist.all_reduce(t, op=ctx.dist.ReduceOp.MAX)
            tuning = {c: float(v) for c, v in zip(candidates, t.tolist())}
        best = min(candidates, key=lambda c: tuning[c])
    else:
        best = candidates[0]

    only_fn = None
    if args.only_mode == "torch_autograd":
        only_fn = lambda q: -0.5 * (q * q * inv_var).sum(-1)  # noqa: E731
    elif args.only_mode == "torch_pair":
        def only_fn(q):
            g = -(q * inv_var)
            return 0.5 * (q * g).sum(-1), g

        bjx.returns_pair(only_fn)
    head = measure(best[0], best[1], args.full, streams=best[2], fn=only_fn,
                   timing=only_fn is None, dump=True)  # THE timed region
    final_draws = ctx.gather_rows(head["state"].position[:256])  # the only thing that crosses xGMI

    # ---- extra regions (rank 0 timing only matters; all ranks run them so barriers line up)
    extras = args.full and not args.headline_only and not args.only_mode
    stream_m = cache_m = None
    # (every rank takes the same branches here: the extra regions contain barriers)
    if head["timed"] and head["streams"] == 1:  # concurrent blocks share the chip: not a clean per-launch time
        if head["chain_block"] >= N:
            stream_m = head
        else:
            cache_m = head
    if extras and not args.no_launch_timing:
        if stream_m is None:
            stream_m = measure(N, False, False)
        if cache_m is None and blk_auto < N:
            cache_m = measure(blk_auto, False, False)

    roofline = None
    if rank == 0 and ((stream_m and stream_m["launch"]) or (cache_m and cache_m["launch"])):
        flat = D % 1024 == 0 and os.environ.get("BJX_LF_FLAT", "1") != "0"
        src = stream_m or cache_m
        la = src["launch"]
        roofline = {"bound": "hbm", "kernel": "k_leapfrog_diag_flat<2>" if flat else "k_leapfrog_diag<4,2>",
                    "achieved": la["achieved"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": la["achieved"] / HBM_PEAK_GBS, "traffic": None, "traffic_source": None,
                    "nontemporal": bool(flat and stream_m is not None and os.environ.get("BJX_LF_NT", "") != "0"
                                        and 12.0 * D * la["chains_per_launch"] > (256 << 20)),
                    "mode": ("hbm streaming: all chains per launch" if stream_m else
                             "Infinity-Cache blocks (no streaming measurement in this run)"),
                    **{k: la[k] for k in ("algorithmic_bytes_per_launch", "chains_per_launch",
                                          "avg_launch_us", "launches_timed", "timed_every")},
                    "region_ms_per_step": src["ms_per_step"]}
        if cache_m is not None and stream_m is not None:
            lc = cache_m["launch"]
            roofline["cache_assisted_achieved"] = lc["achieved"]
            roofline["cache_assisted_frac"] = lc["achieved"] / HBM_PEAK_GBS
            roofline["cache_assisted"] = {
                **lc, "region_ms_per_step": cache_m["ms_per_step"],
                "note": "same kernel on chain blocks whose q/p/g stay in the 256 MiB Infinity Cache across "
                        "the L steps: part of these bytes never reach HBM, so this figure may exceed what "
                        "HBM alone can deliver and is NOT the HBM roofline fraction"}
        tpath = os.path.join(ROOT, "profiles", "traffic_latest.json")
        if os.path.exists(tpath):
            try:
                tj = json.load(open(tpath))
                if tj.get("chains") == N and tj.get("dim") == D:
                    per_chain = tj.get("hbm_bytes_per_launch") / tj.get("chains_per_launch", N)
                    roofline["traffic"] = per_chain * roofline["chains_per_launch"]
                    roofline["traffic_source"] = ("profiles/traffic_latest.json (rocprofv3 --pmc passes of an "
                                                  "earlier run, committed; scaled per chain; NOT measured in "
                                                  "this run; counters sit at the L2 memory-side interface and "
                                                  "include Infinity-Cache hits; passes taken on build: "
                                                  f"{tj.get('measured_on_build', 'round 5 final')})")
                    roofline["traffic_build"] = tj.get("measured_on_build", "round 5 final")
            except Exception:
                pass
        # what an empty event bracket costs, behind a kernel of the same kind
        try:
            empties = []
            probe = torch.zeros(roofline["chains_per_launch"], D, device=dev)
            for _ in range(32):
                probe.add_(1.0)
                s_ev, e_ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s_ev.record()
                e_ev.record()
                empties.append((s_ev, e_ev))
            torch.cuda.synchronize()
            roofline["event_bracket_overhead_us"] = float(np.median([a.elapsed_time(b) for a, b in empties[8:]])) * 1e3
        except Exception:
            pass

    # ---- the user log-density as PyTorch code: the path north_star names.  Three labelled lines:
    #   torch_callable_mode        lambda q: -0.5 * (q*q*inv_var).sum(-1) through torch.autograd (plain launches)
    #   torch_callable_graph_mode  the same callable with the block's inner loop recorded as a HIP graph
    #   torch_pair_mode            a plain-torch (logp, grad) pair: g = -(q*iv); lp = 0.5*(q*g).sum(-1)
    # bytes per element of each callable: measured with rocprofv3 --pmc over `--only-mode ...` runs and
    # committed as profiles/torch_modes_latest.json (read here; estimates are labelled as such otherwise)
    def torch_logdensity(q):
        return -0.5 * (q * q * inv_var).sum(-1)

    def torch_pair(q):
        g = -(q * inv_var)
        return 0.5 * (q * g).sum(-1), g

    bjx.returns_pair(torch_pair)
    measured_bpe = {}
    mpath = os.path.join(ROOT, "profiles", "torch_modes_latest.json")
    if os.path.exists(mpath):
        try:
            measured_bpe = json.load(open(mpath))
        except Exception:
            measured_bpe = {}

    def torch_line(m, k_t, name, logdensity_text, est_callable_bpe):
        pm = measured_bpe.get(name) or {}
        total = pm.get("bytes_per_element_total")  # engine + callable, per chain-leapfrog element
        line = {"value": m["value"], "unit": "chain-leapfrog-steps/s", "ms_per_step": m["ms_per_step"],
                "steps": k_t, "chain_block": m["chain_block"], "hip_graph": m["hip_graph"],
                "logdensity": logdensity_text, "engine_bytes_per_element": 20,
                "callable_bytes_per_element_estimate": est_callable_bpe,
                "bytes_per_element_measured": total,
                "bytes_per_element_source": (pm.get("source") if total else
                                             "estimate (no PMC summary committed for this mode)"),
                "mean_acceptance": m["mean_acceptance"]}
        bpe = total if total else 20.0 + est_callable_bpe
        line["frac_of_roofline_at_those_bytes"] = m["value"] / world / (HBM_PEAK_GBS * 1e9 / (bpe * D))
        return line

    torch_mode = torch_autograd_mode = torch_graph_mode = torch_pair_mode = None
    if extras and not args.no_torch_callable:
        k_t = max(2, args.steps // 4)
        # (0) the DEFAULT path: hmc(torch_logdensity, ...) -- a plain PyTorch function, nothing declared.  Its first call
        # is evaluated under autograd and, since it returns only logp, traced into ONE generated value-and-gradient
        # kernel (blackjax_amd._util._try_elementwise -> targets.from_elementwise), checked against that autograd call.
        def torch_logdensity_default(q):
            return -0.5 * (q * q * inv_var).sum(-1)

        m0 = measure(blk_auto, False, False, steps=k_t, fn=torch_logdensity_default, timing=False)
        vg0 = bjx._util.value_and_grad(torch_logdensity_default)
        traced = [k for k, v in getattr(vg0, "_bjx_elementwise", {}).items() if v is not None]
        torch_mode = torch_line(m0, k_t, "torch_elementwise" if traced else "torch_autograd",
                                "lambda q: -0.5 * (q * q * inv_var).sum(-1) handed to hmc(...) as is", 8 if traced else 48)
        torch_mode["path"] = ("default: traced on first call into one generated HIP value-and-gradient kernel "
                              "(elementwise.from_elementwise), verified against that call's autograd result" if traced
                              else "default: eager torch.autograd (the function is outside the element-wise + row-sum shape)")
        torch_mode["frac_of_28B_roofline"] = m0["value"] / world / (HBM_PEAK_GBS * 1e9 / (28.0 * D))
        # (1) the same function kept on eager autograd (blackjax_amd.no_trace): what the default path saves
        bjx.no_trace(torch_logdensity)
        m = measure(blk_auto, False, False, steps=k_t, fn=torch_logdensity, timing=False)
        # elementwise autograd passes (fp32 words per element): q*q r1 w1, *inv_var r1 w1, sum r1,
        # backward through mul/mul r3 w3 (+ accumulation) -> ~12 words vs 2 for a fused callable
        torch_autograd_mode = torch_line(m, k_t, "torch_autograd",
                                         "lambda q: -0.5 * (q * q * inv_var).sum(-1)  (torch.autograd.grad, grad_outputs=ones)", 48)
        torch_autograd_mode["path"] = "blackjax_amd.no_trace(fn): eager torch.autograd on every call"
        torch_autograd_mode["frac_of_68B_roofline"] = m["value"] / world / (HBM_PEAK_GBS * 1e9 / (68.0 * D))
        torch_autograd_mode["frac_of_28B_roofline"] = m["value"] / world / (HBM_PEAK_GBS * 1e9 / (28.0 * D))
        if world > 1:
            torch_graph_mode = {"value": None, "skipped": "single-GPU runs only (no graph capture under a process group)"}
        else:
            try:
                mg = measure(blk_auto, True, False, steps=k_t, fn=torch_logdensity, timing=False)
                torch_graph_mode = torch_line(mg, k_t, "torch_autograd",
                                              torch_autograd_mode["logdensity"] + ", inner loop as a HIP graph", 48)
            except Exception as e:  # a callable torch cannot record is driven with plain launches: say why
                torch_graph_mode = {"value": None, "error": repr(e)[:300]}
        mp = measure(blk_auto, False, False, steps=k_t, fn=torch_pair, timing=False)
        # g = -(q*iv): r1 w1 (+ neg fused or r1 w1); q*g: r2 w1; sum: r1 -> ~6-8 words
        torch_pair_mode = torch_line(mp, k_t, "torch_pair",
                                     "g = -(q * inv_var); lp = 0.5 * (q * g).sum(-1); return lp, g  (no autograd)", 32)

    # ---- the same plain-PyTorch log-density, (a) traced by blackjax_amd.targets.from_elementwise (torch.fx ->
    # forward-mode derivative -> ONE hiprtc-compiled value-and-gradient kernel, an external callable: 8 B per element),
    # (b) wrapped in torch.compile (Inductor, if it works on this image) -- what a PyTorch user can do about the
    # autograd line above without writing HIP
    torch_elementwise_mode = torch_compile_mode = None
    if extras and not args.no_torch_callable and world > 1:
        # measure() contains barriers: a compile that fails on ONE rank only (ranks racing for the same Inductor / hiprtc
        # cache) would leave the others waiting -- these two modes are single-GPU measurements
        torch_elementwise_mode = torch_compile_mode = {"value": None, "skipped": "single-GPU runs only"}
    elif extras and not args.no_torch_callable:
        k_t = max(2, args.steps // 4)
        try:
            t_c = time.perf_counter()
            ew_fn = bjx.targets.from_elementwise(torch_logdensity, D, device=dev)
            lp_e, g_e = ew_fn(q_init[:256])
            qa = q_init[:256].detach().clone().requires_grad_(True)
            lp_a = torch_logdensity(qa)
            (g_a,) = torch.autograd.grad(lp_a.sum(), qa)
            t_c = time.perf_counter() - t_c
            me = measure(blk_auto, False, False, steps=k_t, fn=ew_fn, timing=False)
            torch_elementwise_mode = torch_line(
                me, k_t, "torch_elementwise",
                "blackjax_amd.targets.from_elementwise(lambda q: -0.5 * (q * q * inv_var).sum(-1), D): the SAME "
                "PyTorch function, traced with torch.fx into one generated HIP value-and-gradient kernel (hiprtc), "
                "called as an external callable between two leapfrogs", 8)
            torch_elementwise_mode.update({
                "generated": ew_fn.elementwise.description, "trace_compile_first_call_s": t_c,
                "max_rel_dgrad_vs_autograd": float(((g_e - g_a).abs() / g_a.abs().clamp_min(1e-30)).max()),
                "max_rel_dlogp_vs_autograd": float(((lp_e - lp_a.detach()).abs() / lp_a.detach().abs().clamp_min(1e-30)).max())})
        except Exception as e:
            torch_elementwise_mode = {"value": None, "error": repr(e)[:300]}
        try:
            t_c = time.perf_counter()
            compiled_pair = torch.compile(torch_pair, dynamic=False)
            bjx.returns_pair(compiled_pair)
            compiled_pair(q_init[:blk_auto])  # compile for the block shape the engine will call it with
            torch.cuda.synchronize()
            t_c = time.perf_counter() - t_c
            mc = measure(blk_auto, False, False, steps=k_t, fn=compiled_pair, timing=False)
            torch_compile_mode = torch_line(mc, k_t, "torch_compile",
                                            "torch.compile(pair) with pair = the torch_pair_mode function (Inductor)", 12)
            torch_compile_mode["compile_s"] = t_c
        except Exception as e:  # Inductor needs a working Triton for gfx950 on this image: report, do not fail
            torch_compile_mode = {"value": None, "error": repr(e)[:300]}

    # ---- what the external-callable contract costs: the same C2 transition with the built-in Gaussian evaluated
    # INSIDE one launch per transition (hmc(..., fuse_target="lean"): engine-resident target, results bit for bit
    # those of the headline path, tests/test_hmc_traj_gpu.py).  NOT the contract, NOT `value`: a labelled line.
    resident_mode = None
    if extras and not args.no_torch_callable:
        try:
            alg_r = bjx.hmc(target, args.eps, imm, L, chain_offset=rank * N, fuse_target="lean")
            st_r = alg_r.init(q_init)
            for t in range(2):
                st_r, inf_r = alg_r.step(keys[t], st_r)
            k_r = max(4, args.steps)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            acc_r = torch.zeros((), device=dev)
            for t in range(k_r):
                st_r, inf_r = alg_r.step(keys[(args.warmup + t) % len(keys)], st_r)
                acc_r += inf_r.acceptance_rate.mean()
            e1.record()
            torch.cuda.synchronize()
            ms_r = e0.elapsed_time(e1) / k_r
            resident_mode = {
                "value": world * N * L / (ms_r * 1e-3), "unit": "chain-leapfrog-steps/s", "ms_per_step": ms_r,
                "steps": k_r, "mean_acceptance": float(acc_r) / k_r,
                "note": "engine-resident target: momentum draw, all L leapfrogs with the Gaussian's (logp, grad) in "
                        "registers, energies and accept in ONE launch per transition (bjx_hmc_trajectory_diag); a "
                        "leapfrog moves no bytes, the launch is bound by the momentum draw's arithmetic.  OUTSIDE "
                        "the external-callable contract -- shown to price that contract, never the headline"}
        except Exception as e:
            resident_mode = {"value": None, "error": repr(e)[:300]}

    # ---- ESS/sec (second half of BASELINE.json's metric)
    def ess_of(draws, dt):
        if len(draws) < 4:
            return None
        e = float(bjx.diagnostics.effective_sample_size(torch.stack(draws, dim=1)).min().item())
        return {"min_ess_subset": e, "subset_chains": n_sub, "draws_per_chain": len(draws),
                "min_ess_per_sec_subset": e / dt,
                "min_ess_per_sec_all_chains": e / dt * (world * N / n_sub)}

    ess = ess_of(head["draws"], head["dt"])
    if ess is not None:
        ess["note"] = ("contract parameters: eps*L = 12.5 is within 0.3 % of 4*pi for the ideal mass matrix "
                       "(leapfrog phase 50 * 2*asin(0.125) = 12.533), so every transition returns each chain "
                       "almost to its start -- this ESS does not grow with the number of draws; see "
                       "ess_nonresonant for a meaningful figure")
    ess_nr = None
    if extras and not args.no_ess_nonresonant and args.steps >= 4:
        m = measure(head["chain_block"], head["hip_graph"], True, eps=0.21, timing=False, streams=head["streams"])
        ess_nr = ess_of(m["draws"], m["dt"])
        if ess_nr is not None:
            ess_nr.update({"eps": 0.21, "leapfrogs": L, "ms_per_step": m["ms_per_step"],
                           "mean_acceptance": m["mean_acceptance"],
                           "note": "same kernels and cost per transition with eps = 0.21: trajectory phase "
                                   "50 * 2*asin(0.105) = 10.5 rad, not a multiple of 2*pi"})

    parity = None
    if rank == 0 and args.full and not args.no_parity and not args.only_mode and not args.headline_only:
        parity = _try_parity(parity_c2, bjx, dev, rank, head["state"], target, imm, inv_var, N, D, L, args.eps,
                             (head["chain_block"], head["hip_graph"], head["streams"]))
    if rank != 0:
        return None
    value = head["value"]
    out = {
        "metric": "chain-leapfrog-steps/sec (whole node), 65 536 chains x 1 024-dim diag-mass HMC",
        "value": value, "unit": "chain-leapfrog-steps/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": head["ms_per_step"], "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {
            "workload": f"C2: HMC diag mass, {N} chains/GPU x {D}-dim Gaussian (sigma ladder 0.1..10), "
                        f"L={L}, eps={args.eps}, user log-density = " +
                        ("HIP DiagGaussian callable" if not args.only_mode else f"PyTorch code ({args.only_mode}; NOT the headline)"),
            "chains_per_gpu": N, "dim": D, "leapfrogs": L, "global_chains": world * N,
            "chain_block": head["chain_block"], "hip_graph": head["hip_graph"], "streams": head["streams"],
            "parallelism": f"chains sharded x{world}, no data-path collective",
        },
        "per_rank_ms_per_step": [p / args.steps * 1e3 for p in head["per_rank_dt"]],
        "gpu_ms_of_each_step": head["gpu_ms_of_each_step"],
        "host_enqueue_ms_per_step": head["host_enqueue_ms_per_step"],
        "host_issue_ms_unthrottled": head["host_issue_ms_unthrottled"],
        "host_note": "host_enqueue_ms_per_step is measured inside the timed region and includes launch calls "
                     "blocking on a full queue (the host runs ahead of the GPU until back-pressure); "
                     "host_issue_ms_unthrottled is the host's own cost of issuing one transition into an empty queue",
        "mean_acceptance": head["mean_acceptance"],
        "ess": ess, "ess_nonresonant": ess_nr,
        "end_to_end_frac_of_28B_roofline": value / world / (HBM_PEAK_GBS * 1e9 / (28.0 * D)),
        "final_draws_gathered": list(final_draws.shape),
        "scheduling_autotune_ms_per_step": {f"chain_block={cb},hip_graph={gr},streams={ns_}": v
                                            for (cb, gr, ns_), v in tuning.items()} or None,
        "torch_callable_mode": torch_mode,
        "torch_autograd_mode": torch_autograd_mode,
        "torch_callable_graph_mode": torch_graph_mode,
        "torch_pair_mode": torch_pair_mode,
        "torch_elementwise_mode": torch_elementwise_mode,
        "torch_compile_mode": torch_compile_mode,
        "engine_resident_target_mode": resident_mode,
        "roofline": roofline,
        "parity": parity,
    }
    return out


# ------------------------------------------------------------------------------------ C4
def bench_c4(args, ctx):
    """configs[3]: window_adaptation(hmc) with per-chain step size and per-chain diagonal inverse
    mass matrix.  W untimed + K timed warm-up steps = two ``run`` calls (the Stan schedule is a
    function of the run's length, so the timed run is a complete K-step warm-up of its own)."""
    import blackjax_amd as bjx
    from blackjax_amd import _lib
    from blackjax_amd.hmc import auto_chain_block

    dev, world, rank = ctx.dev, ctx.world, ctx.rank
    N, D, L = args.chains or 32768, args.dim or 4096, args.leapfrogs
    sig = torch.as_tensor(sigma_ladder(D, -1.5, 1.5), device=dev)
    target = bjx.targets.DiagGaussian((1.0 / (sig * sig)).contiguous())
    gen = torch.Generator(device=dev)
    gen.manual_seed(99 + rank)
    q0 = torch.randn(N, D, device=dev, generator=gen)
    keep = bjx.adaptation.get_filter_adapt_info_fn(info_keys={"acceptance_rate"})
    warm = bjx.window_adaptation(bjx.hmc, target, num_integration_steps=L, adaptation_info_fn=keep)
    blk = min(auto_chain_block(N, D, 4), N)
    timed_kernel = "bjx_leapfrog_diag"

    if args.warmup > 0:
        warm.run(bjx.random.key(1), q0, args.warmup, chain_offset=rank * N)
    torch.cuda.synchronize()
    launches = L * ((N + blk - 1) // blk)
    every = args.time_every or (16 if launches >= 100 else 1)
    timer = None
    if rank == 0 and args.full and not args.no_launch_timing:
        timer = _lib.LaunchTimer([timed_kernel], every, (launches // every + 1) * args.steps)
        torch.cuda.synchronize()
        _lib.set_timer(timer)
    box = {}

    def whole_run(i):
        box["res"] = warm.run(bjx.random.key(2), q0, args.steps, chain_offset=rank * N)

    dt, per, t_enq = timed_region(ctx, whole_run, 1)
    _lib.set_timer(None)
    (state, params), info = box["res"]
    if args.dump_outputs and rank == 0:
        write_outputs(args.dump_outputs, {"state": state, "parameters": params, "info": info}, N)
    acc = info.info.acceptance_rate  # (K, N)
    eps_final = params["step_size"]
    pooled = ctx.gather_rows(torch.stack([eps_final.mean(), eps_final.min(), eps_final.max(),
                                          acc[-1].mean()]).reshape(1, 4))
    # host cost of ISSUING one warm-up step: host_enqueue_ms_per_step below is measured inside
    # the timed region, where launch calls block on a full queue, so it tracks the GPU time.  Here the SAME launch
    # sequence per step (same schedule, same number of chain blocks, L leapfrogs + L callables per block, Welford,
    # dual averaging) runs on 8 chains per block: every launch is a few microseconds of GPU work, so the wall time
    # per step is an UPPER bound of what the host needs to issue a step.
    host_issue_ms = None
    if rank == 0 and args.full:
        try:
            import types

            n_blocks = (N + blk - 1) // blk
            tiny_alg = types.SimpleNamespace(
                init=bjx.hmc.init, build_kernel=lambda integ: bjx.hmc.build_kernel(integ, chain_block=8, use_graph=False))
            warm_t = bjx.window_adaptation(tiny_alg, target, num_integration_steps=L, adaptation_info_fn=keep)
            q_t = q0[:8 * n_blocks].contiguous()
            warm_t.run(bjx.random.key(3), q_t, 3)
            torch.cuda.synchronize()
            k_h = min(40, args.steps)
            t_h = time.perf_counter()
            warm_t.run(bjx.random.key(4), q_t, k_h)
            torch.cuda.synchronize()
            host_issue_ms = (time.perf_counter() - t_h) / k_h * 1e3
        except Exception as e:
            print(f"bench.py: c4 host-issue probe failed: {e!r}", file=sys.stderr)
    if rank != 0:
        return None
    roofline = None
    if timer is not None:
        d_ms = timer.durations_ms(timed_kernel)
        avg_s = float(np.mean(d_ms)) * 1e-3
        alg_bytes = 24.0 * D * min(blk, N)  # read p,g,q,imm (per chain) ; write p,q
        roofline = {"bound": "hbm", "kernel": "k_leapfrog_diag_flat<2> (per-chain inverse mass)",
                    "achieved": alg_bytes / avg_s / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": alg_bytes / avg_s / 1e9 / HBM_PEAK_GBS, "traffic": None,
                    "algorithmic_bytes_per_launch": alg_bytes, "chains_per_launch": min(blk, N),
                    "avg_launch_us": avg_s * 1e6, "launches_timed": len(d_ms), "timed_every": every,
                    "mode": ("Infinity-Cache blocks (chain_block='auto'): part of the traffic is served by "
                             "the cache" if blk < N else "hbm streaming")}
    value = world * N * L * args.steps / dt
    return {
        "metric": "chain-leapfrog-steps/sec (whole node), window_adaptation HMC warm-up, "
                  "32 768 chains/GPU x 4 096-dim",
        "value": value, "unit": "chain-leapfrog-steps/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {
            "workload": f"C4: window_adaptation(hmc, L={L}) on the {D}-dim ill-conditioned Gaussian "
                        f"(sigma 10^-1.5..10^1.5), {N} chains/GPU, per-chain step size and inverse mass "
                        f"matrix, {args.steps}-step Stan schedule",
            "chains_per_gpu": N, "dim": D, "leapfrogs": L, "global_chains": world * N,
            "chain_block": blk, "parallelism": f"chains sharded x{world}, no data-path collective",
        },
        "per_rank_ms_per_step": [p / args.steps * 1e3 for p in per],
        "host_enqueue_ms_per_step": t_enq / args.steps * 1e3,
        "host_issue_ms_unthrottled": host_issue_ms,
        "host_issue_over_ms_per_step": (host_issue_ms / (dt / args.steps * 1e3)) if host_issue_ms else None,
        "host_note": "host_enqueue_ms_per_step is measured inside the timed region and includes launch calls blocking on a "
                     "full queue; host_issue_ms_unthrottled is the wall time per step of the SAME launch sequence on 8 chains "
                     "per block (plain launches): an upper bound of the host's own cost of issuing one warm-up step",
        "end_to_end_frac_of_32B_roofline": value / world / (HBM_PEAK_GBS * 1e9 / (32.0 * D)),
        "adapted": {"per_rank_[mean_eps,min_eps,max_eps,last_step_mean_acceptance]": pooled.tolist()},
        "roofline": roofline,
    }


# ------------------------------------------------------------------------------------ C3
MFMA_F32_PEAK_TFLOPS = 157.3  # /opt/skills/guides/MI355X_MICROARCH.md: dense fp32 matrix peak


def bench_c3(args, ctx, T=None, lockstep_steps=8):
    """configs[2]: NUTS (iterative tree doubling, max_depth = 10) on the 256-dim Neal funnel, 32 768
    chains PER GPU, eps = 0.1, identity metric -- under the external-callable contract (the funnel is
    the library's HIP callable, evaluated between two tick launches; ``fuse_target`` stays off).
    Timed region = ONE ``alg.run(key, state, T)`` (free-running chains: every chain walks through its own
    T trees, NOTEBOOK.md section 7); ``value`` = leapfrogs all chains took / wall.  A second region times
    ``lockstep_steps`` calls of ``alg.step`` (the reference's API: all chains in lockstep)."""
    import blackjax_amd as bjx
    from blackjax_amd import _lib

    dev, world, rank = ctx.dev, ctx.world, ctx.rank
    N, D = args.chains or 32768, args.dim or 256
    T = int(T or args.steps)
    eps, max_depth = 0.1, 10
    # "auto": the HIP-graph drivers for this recordable callable, with their fall-back to plain launches should a
    # capture fail on some rank (a process group's watchdog thread) -- never an exception in a multi-rank run
    alg = bjx.nuts(bjx.targets.NealFunnel(), eps, torch.ones(D, device=dev), max_num_doublings=max_depth,
                   chain_offset=rank * N, use_graph="auto")
    gen = torch.Generator(device=dev)
    gen.manual_seed(rank)
    state = alg.init(0.1 * torch.randn(N, D, device=dev, generator=gen))
    n_warm = max(args.warmup, 4)  # the lockstep driver records one HIP graph per batch bucket on first use
    keys = bjx.random.split(bjx.random.key(0), n_warm + lockstep_steps)
    for t in range(n_warm):
        state, info = alg.step(keys[t], state)
    alg.run(bjx.random.key(5), state, 2, store_positions=False)  # first use of the tick kernels / tail graphs
    torch.cuda.synchronize()
    box = {}

    def whole_run(i):
        box["res"] = alg.run(bjx.random.key(1), state, T, store_positions=False)

    dt, per, _ = timed_region(ctx, whole_run, 1)
    st_run, _, rinfo = box["res"]
    if args.dump_outputs and rank == 0:
        write_outputs(args.dump_outputs, {"state": st_run, "info": rinfo}, N)
    from blackjax_amd import _nuts as _bnuts

    def spec_stats():
        """counters of the run's two-stream speculative tail (include/bjx_nuts.h; empty when it was not taken)"""
        st = dict(_bnuts._SPEC_STATS)
        if st:
            leaves = st["sequences"] * 64
            st["us_per_leapfrog_stream_a"] = st["seconds"] / max(leaves, 1) * 1e6
            st["wasted_share_of_pushed"] = st["stale"] / max(st["pushed"], 1)
        return st or None

    spec_T = spec_stats()
    steps_pc = rinfo.num_integration_steps.sum(0)  # (N,) leapfrogs of each chain over the run
    mine = torch.stack([steps_pc.sum().double(), steps_pc.max().double(),
                        rinfo.num_trajectory_expansions.float().mean().double(),
                        rinfo.is_divergent.float().mean().double()]).reshape(1, 4)
    pooled = ctx.gather_rows(mine)
    tot = float(pooled[:, 0].sum())
    # ticks of the run >= the busiest chain's leapfrogs + ONE tick per transition (a chain finishes a transition in the
    # launch after the one that completed its tree: deferred ends) -- counting leapfrogs alone overstated the
    # utilisation
    ticks = int(pooled[:, 1].max()) + T
    value = tot / dt

    # ---- the tail-heavy regime: T = 400 (from the second hundred transitions on a handful of chains sit in the
    # funnel's mouth and build depth-10 trees at every transition: 97 % of the run is a few live chains)
    t400 = None
    if args.full and world == 1 and not args.no_c3_t400 and N == 32768 and D == 256:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, ri4 = alg.run(bjx.random.key(1), state, 400, store_positions=False)
        torch.cuda.synchronize()
        dt4 = time.perf_counter() - t0
        tot4 = float(ri4.num_integration_steps.sum())
        ticks4 = int(ri4.num_integration_steps.sum(0).max()) + 400  # + one deferred-end tick per transition
        t400 = {"value": tot4 / dt4, "unit": "chain-leapfrog-steps/s", "transitions": 400, "seconds": dt4,
                "ms_per_transition": dt4 / 400 * 1e3, "frac_of_52B_roofline": tot4 / dt4 / (HBM_PEAK_GBS * 1e9 / (52.0 * D)),
                "busiest_chain_leapfrogs": ticks4 - 400, "ticks_lower_bound": ticks4, "tick_period_avg_us": dt4 / max(ticks4, 1) * 1e6,
                "utilisation": tot4 / (N * max(ticks4, 1)), "speculative_tail": spec_stats()}
        del ri4

    # ---- lockstep step(): the only call the reference's API has
    acc = torch.zeros((), device=dev, dtype=torch.float64)
    st_box = {"state": state}

    step_host_ms = []

    def one_step(i):
        t_h = time.perf_counter()
        st, info = alg.step(keys[n_warm + i], st_box["state"])
        st_box["state"] = st
        acc.add_(info.num_integration_steps.sum())
        step_host_ms.append((time.perf_counter() - t_h) * 1e3)  # step() returns when the transition is done (it polls)

    dt_l = None
    if args.full:
        # two untimed calls right before the region: the runs above went through other drivers of the same object, and
        # the first `step` after them re-records its tail sequences (measured: 27-67 ms for that one call, 4.4-8.3 ms after)
        for t in range(2):
            st_w, _ = alg.step(keys[t], st_box["state"])
        del st_w
        dt_l, per_l, _ = timed_region(ctx, one_step, lockstep_steps)
        tot_l = float(ctx.gather_rows(acc.reshape(1, 1)).sum())
    # the same calls on the lockstep tree driver (step_driver="lockstep": rounds 1-4's `step`), rank 0 of a one-GPU run
    lock_cmp = None
    if args.full and world == 1:
        try:
            alg_lock = bjx.nuts(bjx.targets.NealFunnel(), eps, torch.ones(D, device=dev), max_num_doublings=max_depth,
                                chain_offset=rank * N, use_graph="auto", step_driver="lockstep")
            st_k = state
            for t in range(n_warm):
                st_k, _ = alg_lock.step(keys[t], st_k)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st_k, tot_k = state, 0
            infos = []
            for i in range(lockstep_steps):
                st_k, info_k = alg_lock.step(keys[n_warm + i], st_k)
                infos.append(info_k.num_integration_steps)
            torch.cuda.synchronize()
            dt_k = time.perf_counter() - t0
            tot_k = float(torch.stack(infos).sum())
            lock_cmp = {"value": tot_k / dt_k, "ms_per_transition": dt_k / lockstep_steps * 1e3,
                        "same_final_state": bool(torch.equal(st_k.position, st_box["state"].position))}
        except Exception as e:
            print(f"bench.py: c3 lockstep-driver comparison failed: {e!r}", file=sys.stderr)

    # ---- one full-ensemble tick bracketed with HIP events (plain launches, no graph), rank 0
    tick_us = None
    if rank == 0 and args.full and not args.no_launch_timing:
        try:
            alg_t = bjx.nuts(bjx.targets.NealFunnel(), eps, torch.ones(D, device=dev), max_num_doublings=max_depth,
                             chain_offset=rank * N, use_graph=False, run_use_graph=False)
            tick_timer = _lib.LaunchTimer(["bjx_nuts_async_tick"], every=4, capacity=4096)
            _lib.set_timer(tick_timer)
            alg_t.run(bjx.random.key(1), state, 3, store_positions=False)
            torch.cuda.synchronize()
            _lib.set_timer(None)
            d_ms = tick_timer.durations_ms("bjx_nuts_async_tick")[:24]  # the first ticks: every chain has a leaf
            tick_us = float(np.mean(d_ms)) * 1e3 if d_ms else None
        except Exception as e:
            _lib.set_timer(None)
            tick_us = None
            print(f"bench.py: c3 tick bracket failed: {e!r}", file=sys.stderr)
    parity = None
    if rank == 0 and args.full and not args.no_parity:
        parity = _try_parity(parity_c3, bjx, dev, rank, alg, st_box["state"], N, D, eps, max_depth)
    if rank != 0:
        return None
    peak_rate = HBM_PEAK_GBS * 1e9 / (52.0 * D)  # chain-leapfrogs/s per GPU at 52 B per element
    roofline = {
        "bound": "hbm", "kernel": "k_nuts_async_tick3<NI=1, W=4> (leaf + deferred transition ends, one launch per tick) + funnel callable, whole run",
        "achieved": value / world * 52.0 * D / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
        "frac": value / world / peak_rate, "traffic": None,
        "algorithmic_bytes_per_chain_leapfrog": 52.0 * D,
        "algorithmic_note": "SURVEY.md section 8(d): ~13 words per element and chain-leapfrog (leapfrog 7 incl. the "
                            "callable, momentum sum 2, checkpoint write 1, U-turn checkpoint reads ~2, proposal copy <1); "
                            "whole-run figure: useful leapfrogs x 52 B x D / wall, tail of few live chains included",
        "full_ensemble_tick_us": tick_us,
        "full_ensemble_tick_achieved_GBps": (52.0 * D * N / (tick_us * 1e-6) / 1e9) if tick_us else None,
        "full_ensemble_tick_note": "one tick kernel launch (leaf work + the transition ends deferred from the tick before; "
                                   "the callable's launch is outside this bracket) over all chains, first 24 bracketed "
                                   "ticks of a plain-launch run",
    }
    # MEASURED traffic of one busy-phase tick (tick kernel + callable, every chain live): committed PMC passes
    # (tools/pmc_nuts_traffic.sh -> profiles/nuts_traffic_latest.json; FETCH_SIZE doubled per the guide's gfx950 note)
    tpath = os.path.join(ROOT, "profiles", "nuts_traffic_latest.json")
    if os.path.exists(tpath):
        try:
            tj = json.load(open(tpath))
            if tj.get("chains") == N and tj.get("dim") == D:
                both = tj["tick_plus_callable"]
                per_leap = both["measured_bytes"] / N  # bytes per chain-leapfrog, callable included
                roofline.update({
                    "traffic": both["measured_bytes"],
                    "traffic_unit": "bytes per full-ensemble tick (tick kernel + callable launch), L2 memory-side counters",
                    "traffic_bytes_per_chain_leapfrog": per_leap, "traffic_bytes_per_element": per_leap / D,
                    "traffic_over_algorithmic": per_leap / (52.0 * D),
                    "frac_at_measured_bytes": value / world * per_leap / 1e9 / HBM_PEAK_GBS,
                    "busy_phase_tick_GBps_measured": both.get("GBps_measured"),
                    "busy_phase_tick_frac_measured": both.get("frac_of_8TBps_measured"),
                    "traffic_source": "profiles/nuts_traffic_latest.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of an "
                                      "earlier run, committed; NOT measured in this run; Infinity-Cache hits are counted; "
                                      f"passes taken on build: {tj.get('measured_on_build', 'round 5 final')})",
                    "traffic_build": tj.get("measured_on_build", "round 5 final")})
        except Exception:
            pass
    return {
        "metric": "NUTS useful chain-leapfrog-steps/sec (whole node), 32 768 chains x 256-dim funnel",
        "value": value, "unit": "chain-leapfrog-steps/s", "n_gpus": world, "steps": T, "warmup": n_warm,
        "ms_per_step": dt / T * 1e3, "ms_per_transition": dt / T * 1e3, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {
            "workload": f"C3: NUTS (iterative tree doubling, max_depth={max_depth}) on the {D}-dim Neal funnel, "
                        f"{N} chains/GPU, eps={eps}, identity metric, user log-density = HIP NealFunnel callable "
                        f"(external-callable contract), free-running chains alg.run(T={T})",
            "chains_per_gpu": N, "dim": D, "global_chains": world * N, "transitions": T,
            "parallelism": f"chains sharded x{world}, no data-path collective",
        },
        "per_rank_ms_per_step": [p / T * 1e3 for p in per],
        "mean_leapfrogs_per_chain_transition": tot / (world * N * T),
        "ticks": ticks, "utilisation": tot / (world * N * max(ticks, 1)),
        "tick_period_avg_us": dt / max(ticks, 1) * 1e6,
        "mean_depth": float(pooled[:, 2].mean()), "frac_divergent": float(pooled[:, 3].mean()),
        "speculative_tail": spec_T,
        "free_running_T400": t400,
        "lockstep_step": None if dt_l is None else {
            "value": tot_l / dt_l, "unit": "chain-leapfrog-steps/s", "steps": lockstep_steps,
            "ms_per_transition": dt_l / lockstep_steps * 1e3, "host_ms_of_each_call": step_host_ms,
            "mean_leapfrogs_per_chain_transition": tot_l / (world * N * lockstep_steps),
            "frac_of_52B_roofline": tot_l / dt_l / world / peak_rate,
            "step_driver": "auto -> one free-running transition on a persistent workspace (two-stream speculative tail)",
            "lockstep_tree_driver": lock_cmp,
            "note": "alg.step (the reference's kernel API: one transition of every chain per call; a transition lasts as "
                    "long as the deepest tree of the ensemble -- 1 023 dependent leapfrogs of two launches each); the "
                    "key `lockstep_step` is kept from rounds 1-4, when the lockstep tree driver served it"},
        "roofline": roofline,
        "parity": parity,
    }


# ------------------------------------------------------------------------------------ C5
def bench_c5(args, ctx, steps=None):
    """configs[4]: dense mass-matrix HMC on the 512-dim AR(1) Gaussian (Sigma_ij = 0.9^|i-j|), 16 384
    chains PER GPU, L = 20, eps = 0.5; every velocity v = M^-1 p is one fused fp32 MFMA GEMM launch
    (kick prologue, drift epilogue), as is the momentum draw p = L^-T z."""
    import blackjax_amd as bjx
    from blackjax_amd import _lib

    dev, world, rank = ctx.dev, ctx.world, ctx.rank
    N, D, L = args.chains or 16384, args.dim or 512, 20
    K = int(steps or args.steps)
    tgt = bjx.targets.AR1Gaussian(0.9, D)
    cov = tgt.covariance(dev)
    alg = bjx.hmc(tgt, 0.5, cov, L, chain_offset=rank * N)
    gen = torch.Generator(device=dev)
    gen.manual_seed(rank)
    state = alg.init(torch.randn(N, D, device=dev, generator=gen))
    keys = bjx.random.split(bjx.random.key(0), args.warmup + K)
    for t in range(args.warmup):
        state, info = alg.step(keys[t], state)
    torch.cuda.synchronize()
    timer = None
    if rank == 0 and args.full and not args.no_launch_timing:
        timer = _lib.LaunchTimer(["bjx_leapfrog_dense"], every=4, capacity=L * K + 8)
        _lib.set_timer(timer)
    box = {"state": state}
    acc = torch.zeros((), device=dev)

    def one(i):
        st, info = alg.step(keys[args.warmup + i], box["state"])
        box["state"], box["info"] = st, info
        acc.add_(info.acceptance_rate.mean())

    dt, per, _ = timed_region(ctx, one, K)
    _lib.set_timer(None)
    if args.dump_outputs and rank == 0:
        write_outputs(args.dump_outputs, {"state": box["state"], "info": box["info"]}, N)
    parity = None
    if rank == 0 and args.full and not args.no_parity and D == 512:
        parity = _try_parity(parity_c5, bjx, dev, rank, alg, box["state"], N, D, L, 0.5, 0.9)
    if rank != 0:
        return None
    flops = 2.0 * N * D * D
    roofline = None
    if timer is not None:
        d_ms = timer.durations_ms("bjx_leapfrog_dense")
        avg = float(np.mean(d_ms)) * 1e-3
        roofline = {"bound": "mfma", "kernel": "k_dense_gemm_tn8<EPI_DRIFT, kicks> (kick + v = M^-1 p + drift, one launch)",
                    "achieved": flops / avg / 1e12, "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s",
                    "frac": flops / avg / 1e12 / MFMA_F32_PEAK_TFLOPS, "traffic": None,
                    "algorithmic_flops_per_launch": flops, "avg_launch_us": avg * 1e6,
                    "launches_timed": len(d_ms), "timed_every": 4}
        # MEASURED memory traffic of that launch: committed PMC passes (tools/pmc_dense5.sh -> profiles/r05/dense_c5_pmc_v2.json;
        # FETCH_SIZE doubled per the guide's gfx950 note).  An MFMA-bound kernel: the figure shows it is far from the HBM bound.
        tpath = os.path.join(ROOT, "profiles", "r05", "dense_c5_pmc_v2.json")
        if N == 16384 and D == 512 and os.path.exists(tpath):
            try:
                kj = json.load(open(tpath))["kernels"]["fused_tn8<EPI_DRIFT,2>"]
                algorithmic = 4.0 * (5 * N * D + D * D)  # read p, g, q, write p, q (+ the matrix once)
                tb = float(kj["derived"]["hbm_side_bytes"])
                roofline.update({
                    "traffic": tb, "traffic_unit": "bytes per launch, L2 memory-side counters (Infinity-Cache hits are counted)",
                    "algorithmic_bytes_per_launch": algorithmic, "traffic_over_algorithmic": tb / algorithmic,
                    "traffic_GBps_at_this_launch_time": tb / avg / 1e9, "l2_hit_rate": kj["derived"].get("l2_hit_rate"),
                    "traffic_source": "profiles/r05/dense_c5_pmc_v2.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of an "
                                      "earlier run of the same kernel, committed; NOT measured in this run)"})
            except Exception:
                pass
    value = world * N * L * K / dt
    return {
        "metric": "dense-mass HMC chain-leapfrog-steps/sec (whole node), 16 384 chains x 512-dim",
        "value": value, "unit": "chain-leapfrog-steps/s", "n_gpus": world, "steps": K, "warmup": args.warmup,
        "ms_per_step": dt / K * 1e3, "ms_per_transition": dt / K * 1e3, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {
            "workload": f"C5: dense mass-matrix HMC on the {D}-dim correlated Gaussian (AR(1) rho=0.9), {N} chains/GPU, "
                        f"L={L}, eps=0.5, MFMA momentum-resample GEMM + one fused GEMM per leapfrog",
            "chains_per_gpu": N, "dim": D, "leapfrogs": L, "global_chains": world * N,
            "parallelism": f"chains sharded x{world}, no data-path collective",
        },
        "per_rank_ms_per_step": [p / K * 1e3 for p in per],
        "mean_acceptance": float(acc) / K,
        "end_to_end_TFLOPs": value / world * 2.0 * D * D / 1e12,
        "roofline": roofline,
        "parity": parity,
    }


def sub_configs(args, ctx):
    """After the C2 headline (one GPU, default run): BASELINE.json configs[2..4] as labelled sub-objects,
    each with its own timed region (barrier + synchronize on both sides), workload string and roofline."""
    import copy
    import gc

    out = {}

    def run(name, fn, **over):
        a = copy.copy(args)
        a.chains = a.dim = 0
        a.dump_outputs = None  # --dump-outputs is the headline's
        for k, v in over.items():
            setattr(a, k, v)
        gc.collect()
        torch.cuda.empty_cache()
        t0 = time.perf_counter()
        try:
            res = fn(a)
            for k in ("n_gpus", "higher_is_better", "scaling", "vs_baseline", "data"):
                res.pop(k, None)
            res["wall_s_including_warmup"] = time.perf_counter() - t0
            out[name] = res
        except Exception as e:  # a sub-object never fails the headline
            out[name] = {"value": None, "error": repr(e)[:400]}

    # order: the MFMA-bound config right behind the HBM-bound headline, the latency-bound NUTS run after it (a long
    # stretch of few-row launches leaves the chip in a lower power state, and a launch-level figure measured right
    # behind it read 3-5 % low: 86-88 us where the same build measures 82-84 on its own, NOTEBOOK.md section 16)
    run("c5_dense", lambda a: bench_c5(a, ctx), steps=10, warmup=6)
    run("c3_nuts", lambda a: bench_c3(a, ctx), steps=100, warmup=4)
    run("c4_shard", lambda a: bench_c4(a, ctx), steps=200, warmup=3, leapfrogs=50)
    if "c4_shard" in out and out["c4_shard"].get("value") is not None:
        out["c4_shard"]["steps_note"] = ("a complete 200-step Stan schedule (the 1 000-step warm-up of configs[3] is "
                                         "`bench.py --config c4`): 75 fast steps, 75 slow steps in two windows (two metric updates), 50 fast")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # 40 timed transitions = 0.6 s: a single host/driver hiccup (one 28 ms step among 14.5 ms ones was
    # seen in 1 of 8 back-to-back runs) moves a 10-step region by 8 %, a 40-step region by 2 %
    ap.add_argument("--steps", type=int, default=0,
                    help="timed steps (0 = the config's default: c2 40 transitions, c4 the 1 000-step warm-up "
                         "BASELINE.json configs[3] names)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", choices=["c2", "c3", "c4", "c5"], default="c2")
    ap.add_argument("--no-c3-t400", action="store_true", help="c3: skip the 400-transition (tail-heavy) region")
    ap.add_argument("--no-sub-configs", action="store_true",
                    help="c2 default run: skip the C3 / C5 / C4-shard sub-objects")
    ap.add_argument("--chains", type=int, default=0,
                    help="chains PER GPU (0 = the config's: c2 65 536, c3 32 768, c4 32 768, c5 16 384)")
    ap.add_argument("--dim", type=int, default=0, help="0 = the config's: 1 024 / 256 / 4 096 / 512")
    ap.add_argument("--leapfrogs", type=int, default=50)
    ap.add_argument("--eps", type=float, default=0.25)
    ap.add_argument("--chain-block", type=int, default=-1,
                    help="chains per launch: -1 = autotune, 0 = all chains at once, n = n chains")
    ap.add_argument("--use-graph", action="store_true",
                    help="with an explicit --chain-block: the block's inner loop as a HIP graph")
    ap.add_argument("--streams", type=int, default=1,
                    help="chain blocks advanced concurrently on their own HIP streams (c2)")
    ap.add_argument("--headline-only", action="store_true",
                    help="only THE timed region (no roofline/torch-callable/ESS extra regions)")
    ap.add_argument("--no-torch-callable", action="store_true")
    ap.add_argument("--no-ess-nonresonant", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-launch-timing", action="store_true")
    ap.add_argument("--no-parity", action="store_true",
                    help="skip the parity block (one extra transition per config recomputed by the oracle for a spread "
                         "subset of chains, after the timed regions)")
    ap.add_argument("--no-rng-pin", action="store_true",
                    help="skip the jax.random self-check (it only does anything where `import jax` works)")
    ap.add_argument("--only-mode", choices=["torch_autograd", "torch_pair"], default=None,
                    help="c2: run ONLY this user-callable mode as the timed region (for rocprofv3 passes)")
    ap.add_argument("--time-every", type=int, default=0,
                    help="bracket every k-th leapfrog launch with HIP events (0 = 16 for short launches, else 1)")
    ap.add_argument("--full-line", action="store_true",
                    help="print the FULL object (~25 KB) as the stdout line instead of the compact <= 6 KB line "
                         "(the full object always goes to stderr and gpurun_out/bench_full_latest.json)")
    ap.add_argument("--selftest-control-flow", action="store_true",
                    help="CPU-only exercise of the multi-rank control flow (no GPU work, no measurement)")
    ap.add_argument("--full", action="store_true",
                    help="every extra measurement and check besides the headline: launch-timed rooflines, the "
                         "user-callable and ESS regions, parity against the oracle, the CPU baseline, the jax.random "
                         "pin, the C3 / C5 / C4 sub-objects of the default run, the extra regions of c3 / c4 / c5")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed call returned in its last step as DIR/<name>.npy "
                         "(rank 0's chains; large arrays as a fixed sample of chains; at most 64 MB)")
    args = ap.parse_args()
    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    if args.steps < 0:
        ap.error("--steps must be >= 1")
    if args.steps == 0:
        args.steps = {"c2": 40, "c3": 100, "c4": 1000, "c5": 20}[args.config]

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        spawn_ranks(args)  # does not return
    # RCCL prints a five-line banner ("RCCL version : ... Librccl path : ...") to the C library's STDOUT,
    # flushed when the process exits -- i.e. AFTER anything Python printed (seen on MI355X / ROCm 7.0 with a
    # one-rank communicator).  The contract is ONE JSON line on stdout, so with a process group every rank
    # points file descriptor 1 at stderr for the rest of its life and rank 0 writes the JSON line to a
    # duplicate of the original stdout.
    json_fd = None
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 or os.environ.get("BJX_BENCH_FORCE_PG", "0") == "1":
        sys.stdout.flush()
        json_fd = os.dup(1)
        os.dup2(2, 1)

    def emit(obj):
        line = (obj if isinstance(obj, str) else json.dumps(obj)) + "\n"
        if json_fd is None:
            sys.stdout.write(line)
            sys.stdout.flush()
        else:
            os.write(json_fd, line.encode())

    ctx = Ctx(args)
    try:
        if args.selftest_control_flow:
            selftest_control_flow(args, ctx, emit)
            return
        seen = ctx.ranks_seen()
        out = {"c2": bench_c2, "c3": bench_c3, "c4": bench_c4, "c5": bench_c5}[args.config](args, ctx)
        if (args.full and args.config == "c2" and ctx.world == 1 and not ctx.collective and not args.headline_only
                and not args.only_mode and not args.no_sub_configs and args.chains == 0 and args.dim == 0):
            out.update(sub_configs(args, ctx))
        if ctx.rank == 0:
            out["ranks_seen"] = seen
            out["backend"] = ctx.backend
            # n_gpus = DISTINCT devices the ranks ran on (one node: the device string identifies the GPU);
            # "ranks" = processes.  They can only differ under the gloo test knob (several ranks sharing
            # cuda:0 on a one-GPU box); under RCCL that would be a launch error, not a figure to report.
            distinct = len({r["device"] for r in seen})
            out["ranks"] = ctx.world
            out["devices_distinct"] = distinct
            out["n_gpus"] = distinct
            if ctx.backend == "nccl" and distinct != ctx.world:
                raise SystemExit(f"bench.py: {ctx.world} RCCL ranks ran on {distinct} distinct device(s): {seen}")
            if distinct != ctx.world:
                out["n_gpus_note"] = (f"{ctx.world} ranks shared {distinct} device(s) (BJX_BENCH_BACKEND=gloo "
                                      "control-flow test): NOT a multi-GPU figure")
            if args.full and not args.no_rng_pin:
                out["rng_pin"] = rng_pin_check(ctx.dev)
            if args.full:
                out["oracle_pin"] = ("the oracle the parity blocks check against is itself pinned on the reference's own source executed "
                                     "on a stand-in for JAX (tests/refshim; tests/golden/ref_shim_fixtures.json, "
                                     "tests/test_ref_shim_fixtures.py): every discrete outcome equal, positions to ~1e-6; the "
                                     "jax.random bit streams are NOT pinned by that (rng_pin)")
            if args.full and ctx.world == 1 and not args.no_cpu_baseline and args.config == "c2":
                try:
                    out["cpu_baseline"] = cpu_baseline(args.dim or 1024, args.leapfrogs, args.eps)
                except Exception as e:  # the baseline is a reported extra; never fail the GPU number
                    out["cpu_baseline"] = {"value": None, "error": repr(e)}
            if args.full_line:
                emit(out)
            else:
                emit(compact_line(out, write_full_record(out)))
    finally:
        ctx.finish()


if __name__ == "__main__":
    main()
