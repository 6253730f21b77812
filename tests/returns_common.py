"""What the two discounted-returns test files share: the reference's fixture (``tests/golden/returns``, written by
``tools/make_returns_golden.py``), rings that carry its trajectories among random columns, host float64 statistics, and the derived
tolerance of the normalised values.  Not collected by pytest."""
import json
import math
import os
import re

import numpy as np

from tests import helpers as H
from tests import learner_common as LK

FIXTURE = os.path.join(H.ROOT, "tests", "golden", "returns", "ppo_returns.npz")
UNIT = np.float32(0.37)


def chunk():
    """K, the turns per pipeline stage of the kernel (``kReturnsChunk`` in ``sorrel_amd/csrc/returns.h``)."""
    text = open(os.path.join(H.ROOT, "sorrel_amd", "csrc", "returns.h")).read()
    return int(re.search(r"kReturnsChunk = (\d+);", text)[1])


def max_blocks():
    return LK.max_blocks("returns.h", "kReturnsMaxBlocks")


def load_fixture():
    """The reference's trajectories: dicts of T, gamma, rewards, dones, returns (float32) and normalized (float64)."""
    with np.load(FIXTURE) as z:
        params = json.loads(str(z["params"]))
        return [dict(T=p["T"], gamma=float(z[f"gamma_{i}"]), rewards=z[f"rewards_{i}"], dones=z[f"dones_{i}"], returns=z[f"returns_{i}"],
                     normalized=z[f"normalized_{i}"]) for i, p in enumerate(params)]


def random_columns(rng, rows, cols, done_share=0.1):
    """Rewards that are multiples of float32(0.37) (so that products round) and dones on about a tenth of the slots."""
    rewards = (rng.integers(-10, 11, size=(rows, cols)).astype(np.float32) * UNIT).astype(np.float32)
    dones = (rng.random((rows, cols)) < done_share).astype(np.float32)
    return rewards, dones


def ring_arrays(rng, capacity, cols, first, count, planted=()):
    """Host ``rewards`` / ``dones`` ``[capacity, cols]``: random everywhere (the rows outside the segment too: a kernel that reads them
    gets different returns), with each ``(column, rewards, dones)`` of ``planted`` laid along ring rows ``first .. first + count`` (wrapping)."""
    rewards, dones = random_columns(rng, capacity, cols)
    rows = (first + np.arange(count)) % capacity
    for col, r, d in planted:
        rewards[rows, col], dones[rows, col] = r, d
    return rewards, dones


def tolerance(x, axis=None):
    """``8 T 2^-53 (1 + max|x| / (s + 1e-7))`` for the T float64 values one mean / std covers (``axis=0``: per column): the standard
    bound of a length-T float64 sum carried through ``(x - mean) / (std + 1e-7)``."""
    x = np.asarray(x, np.float64)
    T = x.shape[0] if axis == 0 else x.size
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.std(x, axis=axis, ddof=1) if T > 1 else np.full(x.shape[1:] if axis == 0 else (), np.nan)
        return 8 * T * 2.0 ** -53 * (1 + np.abs(x).max(axis=axis) / (s + 1e-7))


def host_stats(x):
    """(mean, unbiased std) of all values of ``x`` in float64 by ``math.fsum``; NaN std for one value."""
    v = np.asarray(x, np.float64).ravel()
    mean = math.fsum(v) / v.size
    std = math.sqrt(math.fsum((v - mean) ** 2) / (v.size - 1)) if v.size > 1 else float("nan")
    return mean, std


def host_normalized(raw, mode):
    """(normalised float64 values, mean, std) of float32 returns ``[count, cols]`` for ``mode`` 'column' / 'all'."""
    x = np.asarray(raw, np.float64)
    if mode == "all":
        mean, std = host_stats(x)
        return (x - mean) / (std + 1e-7), np.float64(mean), np.float64(std)
    stats = [host_stats(x[:, c]) for c in range(x.shape[1])]
    mean, std = np.array([s[0] for s in stats]), np.array([s[1] for s in stats])
    return (x - mean) / (std + 1e-7), mean, std


def assert_normalized(got, want, tol, ctx):
    """``got`` within ``tol`` of ``want`` (float64), NaN exactly where ``want`` is; a float32 ``got`` must be the rounding of SOME
    value inside the band (rounding is monotone), which grants the float32 output nothing beyond its one rounding."""
    got, want = np.asarray(got), np.asarray(want, np.float64)
    assert got.shape == want.shape, f"{ctx}: shape {got.shape}, expected {want.shape}"
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{ctx}: NaN pattern differs"
    tol = np.broadcast_to(np.asarray(tol, np.float64), want.shape)
    ok = ~nan
    if got.dtype == np.float32:
        lo, hi = (want - tol).astype(np.float32), (want + tol).astype(np.float32)
        assert ((got >= lo) & (got <= hi))[ok].all(), f"{ctx}: float32 values outside the rounded band"
    else:
        err = np.abs(got - want)
        assert (err[ok] <= tol[ok]).all(), f"{ctx}: max error {err[ok].max():.3e} against a tolerance of {tol[ok].min():.3e}"
