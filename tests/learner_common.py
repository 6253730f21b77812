"""What the tests of the learner's entry points share (``sgw_sample``, ``sgw_returns``, ``sgw_policy_sample``, ``sgw_ppo_loss``,
``sgw_iqn_loss``, ``sgw_adam_step``, ``sgw_iqn_forward``): guarded device buffers, bit comparisons, the NumPy restatement of the one
block reduction the kernels use (``sorrel_amd/csrc/block_reduce.h``), and the bodies of the descriptor tests."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from sorrel_amd import _native as N
from tests import helpers as H

GUARD = 256
DEV = "cuda:0"
BLOCK = 256                   # threads of a workgroup (kBlock)


class Guarded:
    """Device memory of ``shape`` (or that many elements) between two guards of 0xA5 bytes (the body starts as 0xA5 as well); ``shift``
    bytes move the body off its 256-byte alignment."""

    def __init__(self, torch, shape, np_dtype, shift=0):
        self.shape = tuple(shape) if isinstance(shape, (tuple, list)) else (int(shape),)
        self.np_dtype = np.dtype(np_dtype)
        self.total, self.lo = int(np.prod(self.shape)) * self.np_dtype.itemsize, GUARD + shift
        self.buf = torch.full((self.lo + self.total + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        assert self.buf.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.lo

    def intact(self):
        return bool((self.buf[:self.lo] == 0xA5).all()) and bool((self.buf[self.lo + self.total:] == 0xA5).all())

    def numpy(self):
        """(through a host copy of the bytes: a shifted body is not aligned to its element size)"""
        return self.buf[self.lo:self.lo + self.total].cpu().numpy().copy().view(self.np_dtype).reshape(self.shape)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize]) if x.dtype.kind == "f" else x


def same_bits(got, want, what, ctx="", nan_payloads=False):
    """Equal dtype, shape and bits.  Any NaN equals any NaN (payloads are not part of the contract) unless ``nan_payloads``."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (ctx, what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.kind == "f" and not nan_payloads:
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (ctx, what, "NaN pattern")
        got, want = np.where(nan, 0, got).astype(got.dtype), np.where(nan, 0, want).astype(got.dtype)
    diff = bits(got) != bits(want)
    assert not diff.any(), (ctx, what, f"{int(diff.sum())} of {diff.size} differ, first at {tuple(np.argwhere(diff)[0])}: "
                                       f"{got[diff][0]!r} != {want[diff][0]!r}")


def ulps(a, b):
    """Distance of float32 arrays in units in the last place (NaN against NaN: 0; NaN against a number: a huge count)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)

    def ordered(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)

    d = np.abs(ordered(a) - ordered(b))
    both = np.isnan(a) & np.isnan(b)
    one = np.isnan(a) ^ np.isnan(b)
    return np.where(both, 0, np.where(one, 1 << 40, d))


def tree(red):
    """``block_sum`` of ``[rows, BLOCK]`` lane values, one row per workgroup: lane ``i`` adds lane ``i + s`` for ``s`` = 128, 64 .. 1."""
    red = red.copy()
    assert red.ndim == 2 and red.shape[1] == BLOCK
    s = BLOCK // 2
    while s > 0:
        red[:, :s] = red[:, :s] + red[:, s:2 * s]
        s //= 2
    return red[:, 0]


def max_blocks(header, constant):
    """The grid cap ``constant`` of ``sorrel_amd/csrc/<header>``."""
    text = open(os.path.join(H.ROOT, "sorrel_amd", "csrc", header)).read()
    return int(re.search(constant + r" = (\d+);", text)[1])


def assert_rejected(function, good_desc, change, word):
    """``function(&desc, NULL)`` of ``good_desc`` with ``change`` applied is ``SGW_EINVAL`` and ``sgw_last_error`` names ``word``."""
    for key, value in change.items():
        setattr(good_desc, key, value)
    assert function(C.byref(good_desc), None) == N.EINVAL
    err = N.load().sgw_last_error()
    assert word in err, err


def c_layout(tmp_path, pairs):
    """The C compiler's view of ``pairs`` = ``[(C type name, [field names])]`` of ``include/sgw.h``, from one compile:
    ``{type: {"sizeof": n, field: offset}}``."""
    body = "".join(f'printf("{t} sizeof %zu\\n", sizeof({t}));\n' + "".join(f'printf("{t} {f} %zu\\n", offsetof({t}, {f}));\n' for f in fields)
                   for t, fields in pairs)
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sgw.h"\nint main(){\n' + body + "return 0;}\n")
    subprocess.run(["gcc", "-I", os.path.join(H.ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        t, f, v = line.split()
        out.setdefault(t, {})[f] = int(v)
    return out
