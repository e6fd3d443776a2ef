"""NumPy restatement of mean-field variational inference (TEST INFRASTRUCTURE, in the style of csgld_restatement.py).

Reference functions followed (cited by name: the reference's source is not held next to this file)
* init, step, sample, generate_meanfield_logdensity      blackjax/vi/meanfield_vi.py
* scale_by_adam, sgd                                      optax, as blackjax_amd/optim.py restates them for a scalar

The reference's step differentiates ``kl = mean_s(logq(z_s) - logp(z_s))`` with ``z = mu + exp(rho) * eps`` and, under
``stl_estimator``, ``(mu, rho)`` detached inside ``logq``.  Written out (``G = grad logp(z)``, ``sigma = exp(rho)``):

    logq_s = sum_d(-eps_sd^2 / 2 - rho_d - log(2 pi) / 2)
    STL:      g_mu[d] = mean_s(-eps_sd / sigma_d - G_sd)      g_rho[d] = mean_s(-eps_sd^2 - G_sd sigma_d eps_sd)
    not STL:  g_mu[d] = -mean_s G_sd                           g_rho[d] = -1 - mean_s(G_sd sigma_d eps_sd)

tests/test_meanfield_vi_api.py holds these formulas against ``torch.autograd`` of the reference's literal lines.

House numerics (include/bjx_hip.h "VI").  ``eps = normal(key, (S, D))`` from the key itself; ``sigma = exp_cr(rho)``
(fp64 exponential rounded once to fp32); the draw is ONE fused multiply-add, ``z = fma(sigma, eps, mu)``, not a
multiply then an add.  ``kl``, ``g_mu`` and ``g_rho`` are formed in fp64 from the fp32 ``G``, ``logp``, ``eps`` and
``sigma`` and rounded once.  The optimiser is optim.py's scalar code applied element by element in fp32, the bias
corrections from the host's count; the new parameters are ``p + u`` in fp32.
"""
from __future__ import annotations

from typing import Any, NamedTuple

import numpy as np

from oracle import prng
from oracle.fp import exp_cr, f32, f64, fma32

LOG_2PI = float(np.log(2.0 * np.pi))


class MFVIState(NamedTuple):
    mu: np.ndarray
    rho: np.ndarray
    opt_state: Any


class AdamState(NamedTuple):
    count: int
    mu: tuple
    nu: tuple


# ----------------------------------------------------------------------------- the optimisers, element by element
class Adam:
    """optim._Adam.update on arrays: every operation the scalar code makes, in its order, one fp32 rounding each."""

    def __init__(self, learning_rate, b1=0.9, b2=0.999, eps=1e-8, eps_root=0.0):
        self.learning_rate, self.b1, self.b2 = float(learning_rate), float(b1), float(b2)
        self.eps, self.eps_root = float(eps), float(eps_root)

    def init(self, params):
        return AdamState(0, tuple(np.zeros_like(p, f32) for p in params), tuple(np.zeros_like(p, f32) for p in params))

    def update(self, grads, state, params=None):
        b1, b2 = f32(self.b1), f32(self.b2)
        count = state.count + 1
        c1 = f32(f32(1.0) - f32(np.power(f64(b1), f64(count))))
        c2 = f32(f32(1.0) - f32(np.power(f64(b2), f64(count))))
        us, mus, nus = [], [], []
        for g, m0, v0 in zip(grads, state.mu, state.nu):
            g = np.asarray(g, f32)
            with np.errstate(all="ignore"):
                m = (f32(1.0 - self.b1) * g + b1 * m0).astype(f32)
                v = (f32(1.0 - self.b2) * (g * g) + b2 * v0).astype(f32)
                m_hat, v_hat = (m / c1).astype(f32), (v / c2).astype(f32)
                u = (m_hat / (np.sqrt((v_hat + f32(self.eps_root)).astype(f32)) + f32(self.eps))).astype(f32)
                us.append((f32(-self.learning_rate) * u).astype(f32))
            mus.append(m), nus.append(v)
        return tuple(us), AdamState(count, tuple(mus), tuple(nus))


class SGD:
    def __init__(self, learning_rate):
        self.learning_rate = float(learning_rate)

    def init(self, params):
        return ()

    def update(self, grads, state, params=None):
        return tuple((f32(-self.learning_rate) * np.asarray(g, f32)).astype(f32) for g in grads), state


# ----------------------------------------------------------------------------- sample, kl_and_grad, step
def init(position, optimizer) -> MFVIState:
    mu = np.zeros_like(np.asarray(position, f32))
    rho = np.full_like(mu, f32(-2.0))
    return MFVIState(mu, rho, optimizer.init((mu, rho)))


def noise(key, S: int, D: int) -> np.ndarray:
    return prng.normal(key, (S, D))


def sample(key, mu, rho, num_samples: int = 1) -> np.ndarray:
    mu, rho = np.asarray(mu, f32), np.asarray(rho, f32)
    eps = noise(key, num_samples, mu.shape[0])
    return fma32(exp_cr(rho)[None, :], eps, mu[None, :])


def kl_and_grad_terms(eps, sigma, rho, logp, G, stl_estimator: bool = True):
    """The formulas of the module docstring on fp64 arrays: ``eps``, ``G`` (S, D), ``sigma``, ``rho`` (D,),
    ``logp`` (S,).  -> (kl, g_mu (D,), g_rho (D,))."""
    eps, sigma, rho, logp, G = (np.asarray(a, f64) for a in (eps, sigma, rho, logp, G))
    with np.errstate(all="ignore"):
        logq = np.sum(-0.5 * eps * eps - rho[None, :] - 0.5 * LOG_2PI, axis=1)
        kl = np.mean(logq - logp)
        if stl_estimator:
            g_mu = np.mean(-eps / sigma[None, :] - G, axis=0)
            g_rho = np.mean(-eps * eps - G * sigma[None, :] * eps, axis=0)
        else:
            g_mu = -np.mean(G, axis=0)
            g_rho = -1.0 - np.mean(G * sigma[None, :] * eps, axis=0)
    return kl, g_mu, g_rho


def kl_and_grad(key, mu, rho, logp, grad, stl_estimator: bool = True):
    """-> (kl, g_mu (D,), g_rho (D,)) in fp64 from the fp32 inputs, the noise and ``sigma`` those of ``sample``."""
    del mu  # the gradients do not depend on it: the kernel does not read it either
    rho, G = np.asarray(rho, f32), np.asarray(grad, f32)
    eps = noise(key, G.shape[0], G.shape[1])
    return kl_and_grad_terms(eps, exp_cr(rho), rho, np.asarray(logp, f32), G, stl_estimator)


def step(key, state: MFVIState, logdensity_fn, optimizer, num_samples: int = 5, stl_estimator: bool = True):
    """``logdensity_fn``: z (S, D) fp32 -> (logp (S,), grad (S, D)) fp32.  -> (new state, kl as fp32)."""
    z = sample(key, state.mu, state.rho, num_samples)
    logp, G = logdensity_fn(z)
    kl, g_mu, g_rho = kl_and_grad(key, state.mu, state.rho, logp, G, stl_estimator)
    grads = (g_mu.astype(f32), g_rho.astype(f32))
    updates, opt_state = optimizer.update(grads, state.opt_state, (state.mu, state.rho))
    return MFVIState((state.mu + updates[0]).astype(f32), (state.rho + updates[1]).astype(f32), opt_state), f32(kl)


def meanfield_logdensity(mu, rho, z) -> np.ndarray:
    """generate_meanfield_logdensity(mu, rho)(z) in fp64: the sum of the normal log-pdfs, (S,)."""
    mu, rho, z = (np.asarray(a, f64) for a in (mu, rho, z))
    u = (z - mu) / np.exp(rho)
    return np.sum(-0.5 * u * u - rho - 0.5 * LOG_2PI, axis=-1)


# ----------------------------------------------------------------------------- the convergence case
CONV_D, CONV_S, CONV_STEPS, CONV_LR = 16, 32, 600, 0.05
CONV_M = np.linspace(-2.0, 2.0, CONV_D).astype(f32)
CONV_STD = np.exp(np.linspace(-1.5, 1.0, CONV_D)).astype(f32)
CONV_SEEDS = (101, 102, 103, 104, 105)
# With STL the estimator has no variance at the optimum and a run ends at a floor of fp32 rounding noise, not at a
# statistical error.  Over the five seeds this restatement's worst was max|mu - m| = 2.62e-6 and
# max|rho - log s| = 9.06e-8; rounding reorders between implementations, so a run is bounded at ten times that.
CONV_MU_BOUND, CONV_RHO_BOUND = 10 * 2.62e-6, 10 * 9.06e-8


def gaussian_target(m, s):
    """The diagonal Gaussian N(m, s^2) up to its constant: ``u = (z - m) / s``, ``logp = sum(-u^2 / 2)`` summed in
    fp64 and rounded once, ``grad = -(u / s)``; the element-wise operations in fp32."""
    m, s = np.asarray(m, f32), np.asarray(s, f32)

    def fn(z):
        u = ((np.asarray(z, f32) - m) / s).astype(f32)
        logp = np.sum(-0.5 * u.astype(f64) * u.astype(f64), axis=-1).astype(f32)
        return logp, (-(u / s)).astype(f32)

    return fn


def converge(seed: int, stl_estimator: bool, steps: int = CONV_STEPS):
    """The convergence case from ``prng.key(seed)``, step ``t`` keyed ``split(key, steps)[t]``.
    -> (max|mu - m|, max|rho - log s|, final state)."""
    opt = Adam(CONV_LR)
    fn = gaussian_target(CONV_M, CONV_STD)
    state = init(np.zeros(CONV_D, f32), opt)
    for k in prng.split(prng.key(seed), steps):
        state, _ = step(k, state, fn, opt, CONV_S, stl_estimator)
    return conv_errors(state.mu, state.rho) + (state,)


def conv_errors(mu, rho):
    mu, rho = np.asarray(mu, f64), np.asarray(rho, f64)
    return (float(np.max(np.abs(mu - CONV_M.astype(f64)))),
            float(np.max(np.abs(rho - np.log(CONV_STD.astype(f64))))))


# ----------------------------------------------------------------------------- the case of the full-step tests
FULL_STEPS, FULL_LR = 4, 0.05
# (S, D) -> seed of the four step keys, chosen so that in the restatement every coordinate of both gradients is at
# least 1e-4 in magnitude at every step (test_meanfield_vi_api.py checks it on the CPU): Adam's first update is
# -lr * g / (|g| + eps), which only a gradient next to zero makes sensitive to its last place
FULL_CASES = {(5, 3): 11, (32, 16): 11, (100, 65): 11}


def full_case(S: int, D: int):
    """-> (inverse variances (D,) of the zero-mean diagonal Gaussian target, the step keys (FULL_STEPS, 2))."""
    inv_var = np.linspace(0.5, 2.0, D).astype(f32)
    return inv_var, prng.split(prng.key(FULL_CASES[(S, D)]), FULL_STEPS)
