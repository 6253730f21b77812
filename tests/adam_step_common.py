"""TEST INFRASTRUCTURE ONLY -- ``sgw_adam_step``'s contract (``include/sgw.h``) restated in NumPy, the tolerance formulas of its tests and
the loader of ``tests/golden/adam_step``.

The restatement follows the header line by line: every operation is rounded on its own in the tensors' dtype, the two fused
multiply-adds go through the C library's ``fma`` / ``fmaf`` (NumPy has none), the norm is summed in the kernel's order (a lane's sixteen
elements serially, the halving tree over 256 lanes, chunks serially into tensor sums, tensors lane-strided and the tree again) and a
device step state holds running products.  Every kernel output is compared with it bit for bit.

Tolerances (``u`` is 2^-24 for float32 and 2^-53 for float64; no libm beyond ``sqrt``):

* ``param_tolerance``: against the reference with the reference's own coefficient fed in, ``m'``, ``v'`` and ``t'`` are compared bit for
  bit and ``|p'_kernel - p'_ref| <= 2u (|q| + |p'|)`` with ``q = p' - p``: one rounding of the quotient and one of the sum.
* ``norm_tolerance``: ``|norm - norm_ref| <= (n_total + 4) u norm`` -- torch sums float32 squares in an order of its own.
* ``device_step_tolerance``: a device step state against a step passed by value.  After ``t`` steps the running product ``beta_pow`` and
  ``pow(beta, t)`` are taken to give bias corrections that agree within ``d = 3 t 2^-53`` relative (t - 1 roundings of the product, one
  ulp of ``pow``, one of the subtraction).  ``m'`` and ``v'`` do not depend on the step.  ``step_size = lr / bc1`` then moves by ``d``
  relative and ``bc2_sqrt`` by ``d / 2``.  Two values within ``r`` relative of each other round to values within ``r + 2u``; each further
  operation on such a pair adds the pair's two roundings, ``2u``.  So ``F(-step_size)``: ``d + 2u``; the numerator ``F(-step_size) m'``:
  ``d + 4u``; ``F(bc2_sqrt)``: ``d / 2 + 2u``; ``sqrt(v') / F(bc2_sqrt)``: ``d / 2 + 4u``; plus ``F(eps)`` (same sign, so the relative
  error does not grow): ``d / 2 + 6u``; the quotient ``q``: ``1.5 d + 12u``; and the sum ``p + q`` rounds twice more:
  ``|p'_a - p'_b| <= |q| (1.5 d + 12u) + 2u |p'|``, to first order."""
from __future__ import annotations

import ctypes
import ctypes.util
import functools
import json
import os

import numpy as np

from tests import learner_common as LK
from tests.learner_common import bits, tree  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE_DIR = os.path.join(HERE, "golden", "adam_step")
CHUNK, BLOCK, MAX_BLOCKS, MAX_TENSORS = 4096, 256, 2048, 4096
CLIP_NONE, CLIP_NORM, CLIP_COEF = 0, 1, 2

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.argtypes = [ctypes.c_double] * 3
_libm.fma.restype = ctypes.c_double
_libm.fmaf.argtypes = [ctypes.c_float] * 3
_libm.fmaf.restype = ctypes.c_float
_fma64 = np.frompyfunc(_libm.fma, 3, 1)
_fma32 = np.frompyfunc(_libm.fmaf, 3, 1)


def unit(dtype) -> float:
    return 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53


def fma(a, b, c, dtype):
    """One fused multiply-add per element, in ``dtype``."""
    dtype = np.dtype(dtype)
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype), np.asarray(b, dtype), np.asarray(c, dtype))
    if a.size == 0:
        return np.zeros(a.shape, dtype)
    return np.asarray((_fma32 if dtype == np.float32 else _fma64)(a, b, c), dtype=dtype).reshape(a.shape)


same_bits = functools.partial(LK.same_bits, nan_payloads=True)      # (an optimiser's state: a NaN's payload counts as well)


# ------------------------------------------------------------------------------------------------------------- the norm's order
def chunk_sum(g):
    """S of one chunk: lane t adds the squares of elements 4 (t + 256 r) + e, r = 0..3, e = 0..3, in that order; then the tree."""
    g = np.asarray(g).reshape(-1)
    assert 0 < g.size <= CHUNK
    x = np.zeros(CHUNK, np.float64)
    x[:g.size] = g.astype(np.float64)
    with np.errstate(all="ignore"):
        sq = (x * x).reshape(4, BLOCK, 4)
        acc = np.zeros(BLOCK, np.float64)
        for r in range(4):
            for e in range(4):
                acc = acc + sq[r, :, e]
        return tree(acc[None, :])[0]


def chunks_of(numel: int) -> int:
    return numel // CHUNK + (1 if numel % CHUNK else 0)


def chunk_map(numels, has_grad=None):
    """[(tensor, chunk)] in the image's order, and every tensor's first chunk."""
    out, first = [], []
    for k, n in enumerate(numels):
        first.append(len(out))
        if n > 0 and (has_grad is None or has_grad[k]):
            out.extend((k, j) for j in range(chunks_of(n)))
    return out, first


def tensor_sum(g):
    """Chunks added serially in chunk order; 0 for a tensor that is skipped or empty."""
    if g is None or g.size == 0:
        return 0.0
    flat, s = np.asarray(g).reshape(-1), 0.0
    with np.errstate(all="ignore"):
        for j in range(chunks_of(flat.size)):
            s = s + chunk_sum(flat[j * CHUNK:(j + 1) * CHUNK])
    return s


def merge(sums):
    """Lane i adds S_i, S_(i + 256), ... serially; the tree merges the lanes."""
    lanes = np.zeros(BLOCK, np.float64)
    with np.errstate(all="ignore"):
        for k, s in enumerate(sums):
            lanes[k % BLOCK] = lanes[k % BLOCK] + s
        return tree(lanes[None, :])[0]


def grad_norm(grads) -> float:
    with np.errstate(all="ignore"):
        return float(np.sqrt(merge([tensor_sum(g) for g in grads])))


def clip_coef(norm, max_norm, dtype):
    F = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        c = F(max_norm) / (F(norm) + F(1e-6))
    return F(1) if c > 1 else c


def torch_clip_coef(norm, max_norm, dtype):
    """What clip_grad_norm_ multiplies by, from the norm IT returned (a 0-d tensor of the gradients' dtype), by torch's own lines."""
    import torch

    total = torch.tensor(norm, dtype={np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}[np.dtype(dtype)])
    return torch.clamp(max_norm / (total + 1e-6), max=1.0).numpy()[()]


# ------------------------------------------------------------------------------------------------------------- the step
def bias_by_value(step: int, beta1: float, beta2: float):
    """(bc1, bc2_sqrt) as _single_tensor_adam computes them for a Python-float step."""
    step = float(step)
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    return bias_correction1, bias_correction2 ** 0.5


def fresh_state():
    return (0, 1.0, 1.0)


def advance(state, beta1: float, beta2: float):
    step, b1, b2 = state
    return (step + 1, b1 * beta1, b2 * beta2)


def bias_from_state(state):
    _, b1, b2 = state
    return 1.0 - b1, float(np.sqrt(np.float64(1.0 - b2)))


def restate(tensors, dtype, *, clip_mode=CLIP_NONE, max_norm=1.0, coef=None, beta1=0.9, beta2=0.999, eps=1e-8, tau=0.0, step=None,
            state=None, zero_grads=False):
    """``tensors``: dicts of p, g (or None), m, v, t (or None) and lr.  Returns dict(tensors=the updated copies, norm, c, state)."""
    dtype = np.dtype(dtype)
    F = dtype.type
    assert (step is None) != (state is None)
    if state is not None:
        state = advance(state, beta1, beta2)
        bc1, bc2_sqrt = bias_from_state(state)
    else:
        bc1, bc2_sqrt = bias_by_value(step, beta1, beta2)
    norm, c = float("nan"), F(1)
    if clip_mode == CLIP_NORM:
        norm = grad_norm([t["g"] for t in tensors])
        c = clip_coef(norm, max_norm, dtype)
    elif clip_mode == CLIP_COEF:
        c = F(coef)
    out = []
    with np.errstate(all="ignore"):
        for t in tensors:
            new = {k: (None if v is None else (np.array(v, dtype) if k != "lr" else v)) for k, v in t.items()}
            if t["g"] is not None and t["p"].size:
                p, g, m, v = (np.asarray(t[k], dtype) for k in ("p", "g", "m", "v"))
                ge = g if clip_mode == CLIP_NONE else g * c
                m2 = fma(F(1 - beta1), ge - m, m, dtype)
                v2 = fma(F(1 - beta2) * ge, ge, v * F(beta2), dtype)
                denom = np.sqrt(v2) / F(bc2_sqrt) + F(eps)
                step_size = t["lr"] / bc1
                p2 = p + (F(-step_size) * m2) / denom
                new.update(p=p2, m=m2, v=v2)
                if t.get("t") is not None:
                    new["t"] = F(tau) * p2 + F(1.0 - tau) * np.asarray(t["t"], dtype)
                if zero_grads:
                    new["g"] = np.zeros_like(g)
            out.append(new)
    return dict(tensors=out, norm=norm, c=c, state=state)


# ------------------------------------------------------------------------------------------------------------- tolerances
def param_tolerance(p_new, p_old, dtype):
    p_new, p_old = np.asarray(p_new, np.float64), np.asarray(p_old, np.float64)
    return 2.0 * unit(dtype) * (np.abs(p_new - p_old) + np.abs(p_new))


def norm_tolerance(n_total: int, norm: float, dtype) -> float:
    return (n_total + 4) * unit(dtype) * abs(norm)


def device_step_tolerance(p_new, p_old, t: int, dtype):
    p_new, p_old = np.asarray(p_new, np.float64), np.asarray(p_old, np.float64)
    d, u = 3.0 * t * 2.0 ** -53, unit(dtype)
    return np.abs(p_new - p_old) * (1.5 * d + 12.0 * u) + 2.0 * u * np.abs(p_new)


# ------------------------------------------------------------------------------------------------------------- the fixture
def load_fixture(name: str):
    """``iqn`` or ``ppo``: dict(meta=..., steps=[dict(name -> list of arrays per tensor, norm, ...)])."""
    path = os.path.join(FIXTURE_DIR, name + ".npz")
    with np.load(path, allow_pickle=False) as z:
        meta = json.loads(str(z["params"]))
        steps = []
        for s in range(meta["steps"]):
            step = {}
            sizes = [int(np.prod(shape)) for shape in meta["shapes"]]
            cuts = np.cumsum([0] + sizes)
            for key in meta["per_tensor"]:
                flat = z[f"{key}_{s}"]
                step[key] = [flat[cuts[k]:cuts[k + 1]].reshape(meta["shapes"][k]).copy() for k in range(meta["tensors"])]
            for key in meta["per_step"]:
                step[key] = z[f"{key}_{s}"][()]
            steps.append(step)
    return dict(meta=meta, steps=steps, path=path)


def fixture_tensors(step, lrs, with_target):
    return [dict(p=step["param_before"][k], g=step["grad"][k], m=step["exp_avg_before"][k], v=step["exp_avg_sq_before"][k],
                 t=step["target_before"][k] if with_target else None, lr=lrs[k]) for k in range(len(lrs))]
