"""Variational inference on MI355X behind the ``blackjax.vi`` API surface: ``meanfield_vi`` (a diagonal Gaussian
fitted by stochastic gradient steps on the KL divergence) and ``fullrank_vi`` (the same with a full covariance through
its Cholesky factor).  Pathfinder, SVGD and Schrödinger-Föllmer are out of scope."""
from . import fullrank_vi, meanfield_vi

__all__ = ["meanfield_vi", "fullrank_vi"]
