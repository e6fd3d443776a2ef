"""Variational inference on MI355X behind the ``blackjax.vi`` API surface: ``meanfield_vi`` (a diagonal Gaussian
fitted by stochastic gradient steps on the KL divergence).  Full-rank VI, pathfinder, SVGD and Schrödinger-Föllmer are
out of scope."""
from . import meanfield_vi

__all__ = ["meanfield_vi"]
