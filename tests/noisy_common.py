"""What the tests of ``sgw_noisy_weights`` share: the NumPy restatement of its keyed normals (Philox from the oracle, Box-Muller in float64:
include/sgw.h states the key), the keys and counts the GPU test draws with, and the descriptor builder."""
import numpy as np

from oracle import gridstep_oracle as O
from sorrel_amd import _native as N

MASK = 0xFFFFFFFF
COUNTS = (1, 3, 4, 5, 255, 256, 257, 1025)            # around a Philox block (4), a workgroup's row of blocks (256) and a chunk (1024)
EPS_CAP = 2.0 ** -16                                    # |device eps - float64 restatement|: the issue's derivation (about 6e-6 of error)
EPS_MAX = 5.77                                          # sqrt(48 ln 2) = 5.7683: u1 >= 2^-24
# (seed, draw, tensor_id) of the drawn cases, and the one key of the 2^20 draws of the statistical check
BASE_KEY = (0x1234567887654321, 0x0000000500000003, 7)
OTHER_KEYS = ((0x1234567887654320, 0x0000000500000003, 7), (0x1234567887654321, 0x0000000500000004, 7),
              (0x1234567887654321, 0x0000000600000003, 7), (0x1234567887654321, 0x0000000500000003, 8))
STAT_KEY, STAT_COUNT = (20260, 41, 3), 1 << 20


def keyed_words(seed, draw, tensor_id, count):
    """The uint32 pairs ``(w_a, w_b)`` of elements ``0 .. count``: words (0, 1) of block ``i >> 2`` for ``i & 3`` in (0, 1), words (2, 3) else."""
    i = np.arange(count, dtype=np.uint64)
    blk = i >> np.uint64(2)
    ones = np.ones_like(blk)
    w = O.philox4x32_10(blk, ones * np.uint64(draw & MASK), ones * np.uint64((draw >> 32) & MASK),
                        ones * np.uint64(((tensor_id << 4) | N.STREAM_NOISE) & MASK), seed & MASK, (seed >> 32) & MASK)
    w = [np.asarray(x, dtype=np.uint64) for x in w]
    hi = (i & np.uint64(2)) != 0
    return np.where(hi, w[2], w[0]), np.where(hi, w[3], w[1])


def keyed_normals(seed, draw, tensor_id, count):
    """The definition's normals in float64: ``r cos(2 pi u2)`` for even elements, ``r sin(2 pi u2)`` for odd ones."""
    wa, wb = keyed_words(seed, draw, tensor_id, count)
    u1 = ((wa >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (wb >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    odd = (np.arange(count) & 1) != 0
    return np.where(odd, r * np.sin(2.0 * np.pi * u2), r * np.cos(2.0 * np.pi * u2))


def stat_bounds(n):
    """(|mean| bound, |var - 1| bound) of ``n`` standard normals at five standard errors."""
    return 5.0 / np.sqrt(n), 5.0 * np.sqrt(2.0 / n)


def desc(mode, jobs, seed=0, draw=0):
    """An ``SgwNoisyWeightsDesc`` over ``jobs`` = dicts of the job's fields (pointers as integers)."""
    d = N.SgwNoisyWeightsDesc()
    d.mode, d.num_jobs, d.seed, d.draw = mode, len(jobs), seed & 0xFFFFFFFFFFFFFFFF, draw & 0xFFFFFFFFFFFFFFFF
    for slot, job in zip(d.jobs, jobs):
        for key, value in job.items():
            setattr(slot, key, value)
    return d
