"""The check of tensor arguments that the loss wrappers share (``losses.ppo_loss_terms``, ``losses.iqn_loss_terms``)."""
from __future__ import annotations

import torch


def check_tensors(device, other, *args):
    """Every ``(name, x, dtypes, size)`` of ``args`` in turn: ``TypeError`` unless ``x`` is a tensor of one of ``dtypes``, ``ValueError``
    unless it has ``size`` -- an element count, or a tuple of the shapes allowed --, is contiguous and lies on ``device``, the device of
    ``other`` (the name of the argument they go with).  One call for a wrapper's whole argument list: the wrappers' small shapes are
    bound by the host, where a call per argument shows."""
    for name, x, dtypes, size in args:
        if not torch.is_tensor(x):
            raise TypeError(f"{name} must be a tensor, not {type(x).__name__}")
        if x.dtype not in dtypes:
            raise TypeError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, not {x.dtype}")
        if isinstance(size, int):
            if x.numel() != size:
                raise ValueError(f"{name} has {x.numel()} elements for {size} rows of {other}")
        elif tuple(x.shape) not in size:
            raise ValueError(f"{name} has shape {tuple(x.shape)}; expected {' or '.join(str(list(s)) for s in size)}")
        if not x.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if x.device != device:
            raise ValueError(f"{name} is on {x.device}, {other} on {device}")
