"""blackjax/smc/tuning/from_kernel_info.py: strategies that tune the move from the information it returns."""
from __future__ import annotations

import torch

__all__ = ["update_scale_from_acceptance_rate"]


def update_scale_from_acceptance_rate(scales, acceptance_rates, target_acceptance_rate: float = 0.234):
    """blackjax/smc/tuning/from_kernel_info.py ``update_scale_from_acceptance_rate``:
    ``scales * exp(acceptance_rates - target_acceptance_rate)``, elementwise on tensors of one shape (the scales of
    the particles' random-walk proposals and the acceptance rates they achieved).  Plain tensor arithmetic."""
    if not isinstance(scales, torch.Tensor) or not isinstance(acceptance_rates, torch.Tensor):
        raise TypeError("scales and acceptance_rates must be torch.Tensors")
    if scales.shape != acceptance_rates.shape:
        raise ValueError(f"scales and acceptance_rates must have one shape, got {tuple(scales.shape)} and "
                         f"{tuple(acceptance_rates.shape)}")
    return scales * torch.exp(acceptance_rates - target_acceptance_rate)
