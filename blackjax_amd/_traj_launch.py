"""One launcher per (metric, integrator) for the HMC-family drivers (``hmc``, ``mhmc``, ``dynamic_hmc``, ``dmhmc``).

A driver sequences momentum draw, position updates, the user's callable and a closing launch; WHICH entry point of
libbjxhip serves each of them depends on the metric kind, on whether the integrator is velocity Verlet and on the
sampler (the kernels with per-chain trajectory lengths exist in fewer forms).  That table lives here, once; the dense
half of it is ``blackjax_amd.dense``.  Entry points are not interchangeable even where the arithmetic looks equal
(separately rounded kicks): a launcher picks exactly one per operation.
"""
from __future__ import annotations

import os

import torch

from . import _lib, dense

_FUSE_FIRST = os.environ.get("BJX_HMC_FUSE_FIRST", "1") != "0"  # A/B switch (NOTEBOOK.md section 5)


class Launcher:
    """``general``: the integrator is not velocity Verlet (``kick_c`` = b1 .. b1, ``drift_c`` = a1 ..).  ``sampler``
    selects the position-update entry points:

    =============  ==========================================  =======================================
    sampler        diagonal metric                             dense metric
    =============  ==========================================  =======================================
    hmc, mhmc      ``bjx_leapfrog_diag``; general: ``_coef``   ``bjx_leapfrog_dense`` / ``_dense_pc``;
                                                               general: ``bjx_leapfrog_dense_coef``
    dynamic_hmc    ``bjx_leapfrog_diag`` (no lengths given) /  ``bjx_leapfrog_dense_coef`` (the only
                   ``_masked``; general: ``_coef``             one that takes per-chain lengths)
    dmhmc          ``bjx_leapfrog_diag_coef`` (what            ``bjx_leapfrog_dense_coef``
                   ``bjx_mhmc_step_diag_coef`` re-opens with)
    =============  ==========================================  =======================================
    """

    def __init__(self, metric, kick_c=(0.5, 0.5), drift_c=(1.0,), general=False, sampler="hmc"):
        self.metric, self.diag = metric, metric.kind == "diag"
        self.kick_c, self.drift_c = tuple(float(c) for c in kick_c), tuple(float(c) for c in drift_c)
        self.general, self.sampler = general, sampler
        self.coef = general or sampler == "dmhmc" or (sampler == "dynamic_hmc" and not self.diag)
        if self.diag:
            self.imm_p, self.imm_s = metric.imm.data_ptr(), metric.imm_stride

    def rows(self, sl):
        """The launcher of one chain block: per-chain matrices travel with their chains."""
        m = self.metric
        if m.kind == "dense_pc":
            m = m._replace(imm=m.imm[sl], mass_sqrt_t=m.mass_sqrt_t[sl])
        elif m.imm_stride:
            m = m._replace(imm=m.imm[sl])
        return Launcher(m, self.kick_c, self.drift_c, self.general, self.sampler)

    def fuses_first(self, d):
        """Plain velocity-Verlet trajectory on a diagonal metric with rows long enough for the row-per-wave momentum
        kernel: the first kick + drift ride along with the (RNG-bound) momentum draw (``momentum_kick``)."""
        return self.diag and not self.general and d > 128 and _FUSE_FIRST

    def updates(self, n_steps):
        """``(step, stage, n_kicks, ka, kb, a)`` of every position update of an ``n_steps``-step trajectory of the
        endpoint samplers (generalized_two_stage_integrator, integrators.py:104-150): one ``stage`` launch each; the
        closing kick b_K of a step merges with the opening kick b_1 of the next (two separately rounded fmas), the
        last closing kick is ``finish``'s."""
        kick_c, drift_c = self.kick_c, self.drift_c
        for i in range(n_steps):
            for si, a in enumerate(drift_c):
                if si:
                    yield i, si, 1, kick_c[si], 0.0, a
                elif i:
                    yield i, 0, 2, kick_c[-1], kick_c[0], a
                else:
                    yield 0, 0, 1, kick_c[0], 0.0, a

    def momentum(self, stream, key, off, n, d, p0, ke0):
        """Momentum draw and initial kinetic energy; ``key`` = ``random.key_spec``'s (k0, k1, fold)."""
        k0, k1, fold = key
        if self.diag:
            _lib.call("bjx_hmc_momentum_diag", stream, k0, k1, off, fold, n, d, self.imm_p, self.imm_s,
                      p0.data_ptr(), ke0.data_ptr())
        else:
            dense.momentum(stream, self.metric, k0, k1, off, fold, n, d, p0, ke0)

    def momentum_kick(self, stream, key, off, n, d, eps, eps_pc, q0, g0, p0, ke0, q_out, p_out):
        """``momentum`` and the opening ``stage`` of a velocity-Verlet trajectory in one launch (``fuses_first``)."""
        k0, k1, fold = key
        _lib.call("bjx_hmc_momentum_kick_diag", stream, k0, k1, off, fold, n, d, self.imm_p, self.imm_s, eps,
                  _lib.ptr(eps_pc), q0.data_ptr(), g0.data_ptr(), p0.data_ptr(), ke0.data_ptr(), q_out.data_ptr(),
                  p_out.data_ptr())

    def stage(self, stream, n, d, n_kicks, ka, kb, a, eps, eps_pc, q_in, p_in, g, q_out, p_out=None, n_steps=None,
              step_idx=0):
        """One position update: kicks ``(eps ka) g`` [, ``(eps kb) g``], drift ``(eps a) M^-1 p`` (velocity Verlet
        outside the ``_coef`` entry points: the coefficients are the kernel's own 1/2, 1), for the chains whose
        ``n_steps`` exceeds ``step_idx`` when lengths are given.  Returns the tensor that holds the new momentum: the
        shared-matrix GEMM cannot update p in place.  ``p_out=None``: in place where the kernel can, else a fresh
        buffer."""
        if not self.diag:
            if p_out is None:
                p_out = torch.empty_like(p_in)
            if self.coef:
                return dense.leapfrog_coef(stream, self.metric, n, d, n_kicks, ka, kb, a, eps, eps_pc, q_in, p_in, g,
                                           q_out, p_out, n_steps, step_idx)
            return dense.leapfrog(stream, self.metric, n, d, n_kicks, eps, eps_pc, q_in, p_in, g, q_out, p_out)
        if p_out is None:
            p_out = p_in
        if self.coef:
            _lib.call("bjx_leapfrog_diag_coef", stream, n, d, n_kicks, ka, kb, a, eps, _lib.ptr(eps_pc), self.imm_p,
                      self.imm_s, q_in.data_ptr(), p_in.data_ptr(), g.data_ptr(), q_out.data_ptr(), p_out.data_ptr(),
                      _lib.ptr(n_steps), step_idx)
        elif n_steps is None:
            _lib.call("bjx_leapfrog_diag", stream, n, d, n_kicks, eps, _lib.ptr(eps_pc), self.imm_p, self.imm_s,
                      q_in.data_ptr(), p_in.data_ptr(), g.data_ptr(), q_out.data_ptr(), p_out.data_ptr())
        else:
            _lib.call("bjx_leapfrog_diag_masked", stream, n, d, n_kicks, eps, _lib.ptr(eps_pc), self.imm_p,
                      self.imm_s, q_in.data_ptr(), p_in.data_ptr(), g.data_ptr(), q_out.data_ptr(), p_out.data_ptr(),
                      n_steps.data_ptr(), step_idx)
        return p_out

    def finish(self, stream, key, off, n, d, eps, eps_pc, thr, *t):
        """Closing kick and the accept / reject tail of the endpoint proposal.  ``t``: q0, logp0, g0, ke0, q, logp, g,
        p, p_end, q_new, logp_new, g_new, acc_rate, is_acc, is_div, energy."""
        k0, k1, fold = key
        if not self.diag:
            if self.general:
                dense.finish_coef(stream, self.metric, k0, k1, off, fold, n, d, self.kick_c[-1], eps, eps_pc, thr, *t)
            else:
                dense.finish(stream, self.metric, k0, k1, off, fold, n, d, eps, eps_pc, thr, *t)
            return
        tail = (eps, _lib.ptr(eps_pc), self.imm_p, self.imm_s, thr, *[x.data_ptr() for x in t])
        if self.general:
            _lib.call("bjx_hmc_finish_diag_coef", stream, k0, k1, off, fold, n, d, self.kick_c[-1], *tail)
        else:
            _lib.call("bjx_hmc_finish_diag", stream, k0, k1, off, fold, n, d, *tail)

    def mhmc_step(self, stream, key, off, n, d, step, reopen, eps, eps_pc, thr, logp0, ke0, q, p, g, logp, *acc,
                  n_steps=None):
        """Closing kick b1 and reservoir step ``step`` of the multinomial proposal; ``reopen``: the opening kick +
        drift (b1, a1) of the next step as well -- inside the diagonal kernels, as a ``stage`` launch from the fully
        kicked momentum for a dense metric.  Returns the tensor that holds the momentum the next launch reads.
        ``acc``: weight, slpa, any_div, ever, pq, pp, pg, plogp, penergy; ``n_steps``: per-chain lengths (dmhmc)."""
        k0, k1, fold = key
        b1, a1 = self.kick_c[0], self.drift_c[0]
        if not self.diag:
            p1 = dense.mhmc_step(stream, self.metric, k0, k1, off, fold, n, d, step, eps, eps_pc, thr, logp0, ke0, q,
                                 p, g, logp, *acc, n_steps=n_steps, kick_coef=b1 if self.general else None)
            if not reopen:
                return p1
            # velocity Verlet re-uses the half-kicked momentum's buffer (the step kernel has consumed it)
            return self.stage(stream, n, d, 1, b1, 0.0, a1, eps, eps_pc, q, p1, g, q, None if self.general else p,
                              n_steps, 0 if n_steps is None else step + 1)
        args = (stream, k0, k1, off, fold, n, d, step, 1 if reopen else 0, eps, _lib.ptr(eps_pc), self.imm_p,
                self.imm_s, thr, logp0.data_ptr(), ke0.data_ptr(), q.data_ptr(), p.data_ptr(), g.data_ptr(),
                logp.data_ptr(), *[x.data_ptr() for x in acc])
        if self.coef:
            _lib.call("bjx_mhmc_step_diag_coef", *args, _lib.ptr(n_steps), b1, a1)
        else:
            _lib.call("bjx_mhmc_step_diag", *args)
        return p

    def mhmc_finish(self, stream, n, d, L, n_steps, *t):
        """Multinomial proposal: acceptance rate and the L = 0 / never-updated chains (``n_steps``: the masked
        variant, per-chain lengths instead of ``L``).  ``t``: q0, p0, g0, logp0, ke0, ever, slpa, pq, pp, pg, plogp,
        penergy, acc_rate."""
        ptrs = [x.data_ptr() for x in t]
        if n_steps is None:
            _lib.call("bjx_mhmc_finish", stream, n, d, L, *ptrs)
        else:
            _lib.call("bjx_mhmc_finish_masked", stream, n, d, n_steps.data_ptr(), *ptrs)
