"""blackjax_amd -- MI355X-native HMC/NUTS engine behind the blackjax.hmc / blackjax.nuts /
blackjax.window_adaptation API surface (blackjax/__init__.py:70-80,104-112).

Positions are batched ``(n_chains, dim)`` float32 ROCm tensors; the log-density is a
PyTorch callable over the batch; all sampler arithmetic runs in hand-written HIP
kernels (``libbjxhip.so``, C ABI in ``include/bjx_hip.h``).  There is no CPU fallback.
"""
from __future__ import annotations

import functools as _functools

from . import barker as _barker
from . import dynamic_hmc as _dynamic_hmc
from . import elliptical_slice as _elliptical_slice
from . import ghmc as _ghmc
from . import hmc as _hmc
from . import irmh as _irmh
from . import mala as _mala
from . import marginal_latent_gaussian
from . import nuts as _nuts
from . import periodic_orbital
from . import adaptation, chees, diagnostics, distributed, integrators, meads, metrics, optim, random, random_walk, rtc, sgmcmc, smc, targets, util, vi
from .adaptation import staged_adaptation, window_adaptation
from .chees import chees_adaptation
from .meads import meads_adaptation
from .base import AdaptationAlgorithm, SamplingAlgorithm, VIAlgorithm
from ._util import capturable, no_trace, returns_pair

__version__ = "0.1.0"


class GenerateSamplingAPI:
    """blackjax/__init__.py:70-80: callable that also exposes ``init`` / ``build_kernel``."""

    def __init__(self, differentiable, init, build_kernel):
        self.differentiable = differentiable
        self.init = init
        self.build_kernel = build_kernel

    def __call__(self, *args, **kwargs) -> SamplingAlgorithm:
        return self.differentiable(*args, **kwargs)


class GenerateVariationalAPI:
    """blackjax/__init__.py ``GenerateVariationalAPI``: callable that also exposes ``init`` / ``step`` / ``sample``."""

    def __init__(self, differentiable, init, step, sample):
        self.differentiable = differentiable
        self.init = init
        self.step = step
        self.sample = sample

    def __call__(self, *args, **kwargs) -> VIAlgorithm:
        return self.differentiable(*args, **kwargs)


hmc = GenerateSamplingAPI(_hmc.as_top_level_api, _hmc.init, _hmc.build_kernel)
nuts = GenerateSamplingAPI(_nuts.as_top_level_api, _nuts.init, _nuts.build_kernel)
# blackjax/__init__.py:145-151: multinomial HMC shares HMCState / init with hmc
mhmc = GenerateSamplingAPI(
    _functools.partial(_hmc.as_top_level_api, build_proposal=_hmc.multinomial_hmc_proposal),
    _hmc.init,
    _functools.partial(_hmc.build_kernel, build_proposal=_hmc.multinomial_hmc_proposal),
)
multinomial_hmc = mhmc
dynamic_hmc = GenerateSamplingAPI(_dynamic_hmc.as_top_level_api, _dynamic_hmc.init,
                                  _dynamic_hmc.build_kernel)
# batched counterparts of the reference's default callables (dynamic_hmc.py:69-70) + key seeding
dynamic_hmc.next_key_fn = _dynamic_hmc.next_key_fn
dynamic_hmc.randint_steps_fn = _dynamic_hmc.randint_steps_fn
dynamic_hmc.chain_keys = _dynamic_hmc.chain_keys
dynamic_hmc.halton_sequence = _dynamic_hmc.halton_sequence
dynamic_hmc.halton_steps_fn = _dynamic_hmc.halton_steps_fn
dhmc = dynamic_hmc  # blackjax/__init__.py alias used by the ChEES examples
# blackjax/__init__.py:155-163: dynamic trajectory lengths with the multinomial (whole-trajectory) proposal
dmhmc = GenerateSamplingAPI(
    _functools.partial(_dynamic_hmc.as_top_level_api, build_proposal=_hmc.multinomial_hmc_proposal),
    _dynamic_hmc.init,
    _functools.partial(_dynamic_hmc.build_kernel, build_proposal=_hmc.multinomial_hmc_proposal),
)
hmc_family = [hmc, nuts, mhmc]  # blackjax/__init__.py:188
# Generalized HMC (blackjax/mcmc/ghmc.py), the sampler the MEADS warm-up tunes
ghmc = GenerateSamplingAPI(_ghmc.as_top_level_api, _ghmc.init, _ghmc.build_kernel)
# Metropolis-adjusted Langevin (blackjax/mcmc/mala.py): one gradient per transition
mala = GenerateSamplingAPI(_mala.as_top_level_api, _mala.init, _mala.build_kernel)
# Periodic orbital MCMC (blackjax/mcmc/periodic_orbital.py, exported by the reference as orbital_hmc): the state is a
# weighted orbit of `period` samples, rebuilt from one momentum draw by one log-density call on N * period rows
orbital_hmc = GenerateSamplingAPI(periodic_orbital.as_top_level_api, periodic_orbital.init,
                                  periodic_orbital.build_kernel)
# Barker proposal (blackjax/mcmc/barker.py, exported by the reference as barker_proposal): one gradient per
# transition, step size and diagonal metric tuned by window_adaptation
barker = GenerateSamplingAPI(_barker.as_top_level_api, _barker.init, _barker.build_kernel)
barker_proposal = barker
# Elliptical slice sampling (blackjax/mcmc/elliptical_slice.py): Gaussian prior, value-only log-likelihood, no gradient
elliptical_slice = GenerateSamplingAPI(_elliptical_slice.as_top_level_api, _elliptical_slice.init,
                                       _elliptical_slice.build_kernel)
# Marginal latent-Gaussian sampler (blackjax/mcmc/marginal_latent_gaussian.py): Gaussian prior, log-likelihood with a
# gradient, proposal preconditioned by the prior covariance; one gradient per transition, no host read
mgrad_gaussian = GenerateSamplingAPI(marginal_latent_gaussian.as_top_level_api, marginal_latent_gaussian.init,
                                     marginal_latent_gaussian.build_kernel)
# Random-walk Metropolis (blackjax/mcmc/random_walk.py, irmh.py): gradient-free, value-only log-density.  rmh takes any
# batched proposal generator, additive_step_random_walk adds a random step (normal_random_walk: the fused Gaussian
# step), irmh proposes independently of the position
rmh = GenerateSamplingAPI(random_walk.rmh_as_top_level_api, random_walk.init, random_walk.build_rmh)
additive_step_random_walk = GenerateSamplingAPI(random_walk.additive_step_random_walk, random_walk.init,
                                                random_walk.build_additive_step)
additive_step_random_walk.normal_random_walk = random_walk.normal_random_walk
normal_random_walk = random_walk.normal_random_walk
irmh = GenerateSamplingAPI(_irmh.as_top_level_api, _irmh.init, _irmh.build_kernel)
# Tempered SMC (blackjax/smc/tempered.py, adaptive_tempered.py): the particles are the chain batch, the move is
# num_mcmc_steps transitions of the samplers above, resampling / reweighting / the ESS solve are HIP kernels
tempered_smc = GenerateSamplingAPI(smc.tempered.as_top_level_api, smc.tempered.init, smc.tempered.build_kernel)
adaptive_tempered_smc = GenerateSamplingAPI(smc.adaptive_tempered.as_top_level_api, smc.adaptive_tempered.init,
                                            smc.adaptive_tempered.build_kernel)
# Persistent-sampling SMC (blackjax/smc/persistent_sampling.py, adaptive_persistent_sampling.py): every iteration weighs
# the particles of all earlier ones; the mixture denominator, the grid-wide log-sum-exp and the ESS solve are HIP kernels
persistent_sampling_smc = GenerateSamplingAPI(smc.persistent_sampling.as_top_level_api, smc.persistent_sampling.init,
                                              smc.persistent_sampling.build_kernel)
adaptive_persistent_sampling_smc = GenerateSamplingAPI(smc.adaptive_persistent_sampling.as_top_level_api,
                                                       smc.adaptive_persistent_sampling.init,
                                                       smc.adaptive_persistent_sampling.build_kernel)
# Inner-kernel tuning (blackjax/smc/inner_kernel_tuning.py): tempered / adaptive tempered SMC whose move's parameters are
# re-estimated after every temperature (smc.tuning: column moments of the particles are a HIP kernel)
inner_kernel_tuning = GenerateSamplingAPI(smc.inner_kernel_tuning.as_top_level_api, smc.inner_kernel_tuning.init,
                                          smc.inner_kernel_tuning.build_kernel)
# Pretuning (blackjax/smc/pretuning.py): tempered / adaptive tempered SMC with one parameter value per particle; before
# every step the values are scored by the ESJD of a trial transition, jittered and resampled (three HIP kernels)
pretuning = GenerateSamplingAPI(smc.pretuning.as_top_level_api, smc.pretuning.init, smc.pretuning.build_kernel)
# Stochastic-gradient MCMC (blackjax/sgmcmc/sgld.py, sghmc.py, sgnht.py, csgld.py): the gradient is a minibatch estimate
# from the user's callable, the noise draw + diffusion update (+ thermostat) is one fused launch per step; csgld adds
# one launch for its per-chain energy histogram
sgld = GenerateSamplingAPI(sgmcmc.sgld.as_top_level_api, sgmcmc.sgld.init, sgmcmc.sgld.build_kernel)
sghmc = GenerateSamplingAPI(sgmcmc.sghmc.as_top_level_api, sgmcmc.sghmc.init, sgmcmc.sghmc.build_kernel)
sgnht = GenerateSamplingAPI(sgmcmc.sgnht.as_top_level_api, sgmcmc.sgnht.init, sgmcmc.sgnht.build_kernel)
csgld = GenerateSamplingAPI(sgmcmc.csgld.as_top_level_api, sgmcmc.csgld.init, sgmcmc.csgld.build_kernel)
# Mean-field variational inference (blackjax/vi/meanfield_vi.py): a diagonal Gaussian fitted by stochastic gradient steps
# on the KL estimate; the draw, the reduction of the (S, D) gradients and the optimiser updates are HIP kernels
meanfield_vi = GenerateVariationalAPI(vi.meanfield_vi.as_top_level_api, vi.meanfield_vi.init, vi.meanfield_vi.step,
                                      vi.meanfield_vi.sample)
# Full-rank variational inference (blackjax/vi/fullrank_vi.py): a Gaussian with a Cholesky-factored covariance; the
# triangular product of the draw, the batched triangular solve and the outer-product reduction are HIP kernels
fullrank_vi = GenerateVariationalAPI(vi.fullrank_vi.as_top_level_api, vi.fullrank_vi.init, vi.fullrank_vi.step,
                                     vi.fullrank_vi.sample)

__all__ = ["hmc", "nuts", "mhmc", "hmc_family", "multinomial_hmc", "dynamic_hmc", "dhmc", "dmhmc", "ghmc", "mala", "orbital_hmc", "periodic_orbital", "barker", "barker_proposal", "elliptical_slice", "mgrad_gaussian", "marginal_latent_gaussian", "rmh", "irmh", "additive_step_random_walk", "normal_random_walk", "random_walk", "tempered_smc", "adaptive_tempered_smc", "persistent_sampling_smc", "adaptive_persistent_sampling_smc", "inner_kernel_tuning", "pretuning", "smc", "sgld", "sghmc", "sgnht", "csgld", "sgmcmc", "meanfield_vi", "fullrank_vi", "vi", "window_adaptation", "staged_adaptation", "chees_adaptation", "meads_adaptation", "chees", "meads", "optim", "adaptation", "diagnostics", "distributed", "util", "metrics", "integrators", "random", "rtc", "targets", "SamplingAlgorithm", "AdaptationAlgorithm", "VIAlgorithm", "capturable", "returns_pair", "no_trace"]
