"""The checks of tensor arguments: ``check_tensors`` for the loss wrappers' argument lists (``losses.ppo_loss_terms``,
``losses.iqn_loss_terms``), ``check_tensor`` / ``tensor_ok`` for every tensor ``GridEngine`` hands to the library as a raw pointer."""
from __future__ import annotations

import torch


def tensor_ok(x, dtype, size, device) -> bool:
    """Whether ``x`` is a contiguous ``dtype`` tensor on ``device`` of ``size``: an int is the element count; a tuple the exact shape, with
    ``None`` for an extent that is free; a tuple that ends in ``...`` the leading extents of a shape that may go on."""
    if not torch.is_tensor(x) or x.dtype != dtype or x.device != device or not x.is_contiguous():
        return False
    if size.__class__ is int:
        return x.numel() == size
    shape = x.shape
    if size and size[-1] is ...:
        size = size[:-1]
        shape = shape[:len(size)]
    return shape == size or (len(shape) == len(size) and all(w is None or w == g for w, g in zip(size, shape)))


def refuse(name, x, dtype, want, device):
    """The one wording of a refused tensor: what was wanted (``want``: the size in words) and what came."""
    if torch.is_tensor(x):
        got = f"{tuple(x.shape)} {x.dtype} on {x.device}{'' if x.is_contiguous() else ', not contiguous'}"
    else:
        got = type(x).__name__
    raise ValueError(f"{name} must be a contiguous {dtype} tensor of {want} on {device}; got {got}")


def check_tensor(name, x, dtype, size, device):
    """``x`` itself where ``tensor_ok(x, dtype, size, device)``, else ``ValueError`` (for the dtype too: what the engine's callers
    catch).  A kernel that gets ``x.data_ptr()`` reads or writes exactly ``size`` elements of ``dtype`` there: anything else would be an
    out-of-bounds device access."""
    if not tensor_ok(x, dtype, size, device):
        if size.__class__ is int:
            want = f"{size} elements"
        else:
            want = "shape [" + ", ".join("..." if w is ... else "*" if w is None else str(w) for w in size) + "]"
        refuse(name, x, dtype, want, device)
    return x


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
