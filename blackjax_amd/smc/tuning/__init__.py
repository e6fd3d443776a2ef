"""Parameter updates for ``blackjax_amd.smc.inner_kernel_tuning`` behind ``blackjax.smc.tuning``: ``from_particles``
(moments of the particle cloud) and ``from_kernel_info`` (the move's acceptance rates)."""
from . import from_kernel_info, from_particles

__all__ = ["from_kernel_info", "from_particles"]
