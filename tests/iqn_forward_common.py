"""What the two sgw_iqn_forward test files (and ``tools/make_iqn_forward_golden.py``) share: ``fmaf`` restated in NumPy, the NumPy
restatement of the semantics stated in ``include/sgw.h`` (every dot product ONE fused multiply-add chain over k ascending that starts at
the bias), the keyed taus, the BOUND against the reference as a formula, the reference's fixture
(``tests/golden/iqn_forward/forward.npz``) and small helpers.  Not collected by pytest.

* Every kernel output is compared with the restatement BIT FOR BIT, fed the kernel's own ``out_cos`` and taus: ``cosf`` is the one
  library call and cannot be restated; everything behind it can.
* Against the reference (torch on the CPU, which sums in its own order, fused or not): for a dot product of K terms plus a bias in ANY
  order, with or without fused multiply-adds, the error is at most ``gamma(K + 1) (|w| . |x| + |b|)``, ``gamma(n) = n u / (1 - n u)``,
  ``u = 2^-24``.  ``bound`` propagates that in float64 through the layers (relu is 1-Lipschitz; the product ``z`` takes the usual three
  terms plus one rounding; the means are K-term sums and one rounding for the division), with the elementwise difference between the
  two sides' ``cos`` as the input error.  Each side lies within that ``E`` of the exact value: the tolerance between them is ``2 E``."""
import ctypes
import json
import os

import numpy as np

from oracle import gridstep_oracle as O
from tests import helpers as H
from tests.iqn_loss_common import bits, same_bits  # noqa: F401

FIXTURE = os.path.join(H.ROOT, "tests", "golden", "iqn_forward", "forward.npz")
STREAM_TAU = 11
N_COS = 64
U = 2.0 ** -24
F32 = np.float32
WEIGHTS = ("w_head", "b_head", "w_cos", "b_cos", "w_ff", "b_ff", "w_adv", "b_adv", "w_val", "b_val")
# (D, L, N, A, B)
SETS = ((3, 1, 1, 1, 2), (7, 5, 2, 3, 9), (65, 33, 13, 5, 9), (875, 250, 12, 4, 8))


def gamma(n):
    return n * U / (1.0 - n * U)


# ---------------------------------------------------------------------------------------------------------------------------- fmaf
def fmaf(a, b, c):
    """``fmaf`` of float32 arrays (Python 3.10 has no ``math.fma``): the float64 product of two float32 numbers is exact; the addend is
    added with TwoSum; where that sum is inexact and its float64 mantissa is even it moves one ulp toward the residual (round to odd);
    then one rounding to float32."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c = c.astype(np.float64)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
        move = np.isfinite(s) & (err != 0) & even & np.isfinite(err)
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(move, np.nextafter(s, toward), s)
        return s.astype(F32)


def libm_fmaf():
    lib = ctypes.CDLL("libm.so.6")
    lib.fmaf.argtypes = [ctypes.c_float] * 3
    lib.fmaf.restype = ctypes.c_float
    return lib.fmaf


def relu(x):
    """``x > 0 ? x : (x != x ? x : +0)``"""
    x = np.asarray(x)
    return np.where(x > 0, x, np.where(x != x, x, x.dtype.type(0.0)))


def chain(x, w, b):
    """``[M, K] x [J, K] -> [M, J]``: element (m, j) is fmaf(x_K-1, w_K-1, ... fmaf(x_0, w_0, b_j))."""
    x, w, b = np.asarray(x, F32), np.asarray(w, F32), np.asarray(b, F32)
    acc = np.broadcast_to(b[None, :], (x.shape[0], w.shape[0])).astype(F32)
    for k in range(x.shape[1]):
        acc = fmaf(x[:, k, None], w[None, :, k], acc)
    return acc


def pis():
    """``(float)(M_PI * i)``, i = 1..64: what ``torch.FloatTensor([np.pi * i ...])`` holds."""
    return np.array([np.pi * i for i in range(1, N_COS + 1)], np.float64).astype(F32)


def cos_args(taus):
    taus = np.asarray(taus, F32)
    return (taus.reshape(taus.shape[0], -1, 1) * pis()[None, None, :]).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------------- restatement
def restate(w, states, cos):
    """The header's arithmetic behind ``cos`` (float32 ``[B, N, 64]``): ``w`` maps the ten names of ``WEIGHTS`` to the effective weights,
    ``states`` is ``[B, D]`` (float32 or uint8).  Returns ``quantiles [B, N, A]`` and ``qvalues [B, A]`` (float32)."""
    x = np.asarray(states).astype(F32)
    cos = np.asarray(cos, F32)
    B, N = cos.shape[0], cos.shape[1]
    A = np.asarray(w["w_adv"]).shape[0]
    with np.errstate(all="ignore"):
        h = relu(chain(x, w["w_head"], w["b_head"]))
        e = relu(chain(cos.reshape(B * N, N_COS), w["w_cos"], w["b_cos"]))
        z = (np.repeat(h, N, axis=0) * e).astype(F32)
        y = relu(chain(z, w["w_ff"], w["b_ff"]))
        adv = chain(y, w["w_adv"], w["b_adv"])
        val = chain(y, np.asarray(w["w_val"], F32).reshape(1, -1), np.asarray(w["b_val"], F32).reshape(1))
        s = adv[:, 0].copy()
        for a in range(1, A):
            s = s + adv[:, a]
        mean = s / F32(A)
        quant = ((val + adv) - mean[:, None]).astype(F32).reshape(B, N, A)
        t = quant[:, 0, :].copy()
        for q in range(1, N):
            t = t + quant[:, q, :]
        qv = (t / F32(N)).astype(F32)
    return quant, qv


def bound(w, states, cos, cos_other=None):
    """The exact forward in float64 from ``cos`` and the bound ``E`` of the docstring: ``(quantiles64, qvalues64, E_quantiles, E_qvalues)``.
    ``cos_other``: the other side's cosines (their difference is the input error; None: 0)."""
    f = np.float64
    x = np.asarray(states).astype(f)
    c = np.asarray(cos).astype(f)
    B, N = c.shape[0], c.shape[1]
    c = c.reshape(B * N, N_COS)
    dc = np.zeros_like(c) if cos_other is None else np.abs(c - np.asarray(cos_other).astype(f).reshape(B * N, N_COS))
    W = {k: np.asarray(v).astype(f) for k, v in w.items()}
    W["w_val"], W["b_val"] = W["w_val"].reshape(1, -1), W["b_val"].reshape(1)
    D, L, A = x.shape[1], W["w_ff"].shape[0], W["w_adv"].shape[0]

    def layer(xv, ex, wk, bk, K):
        pre = xv @ W[wk].T + W[bk]
        mag = (np.abs(xv) + ex) @ np.abs(W[wk]).T + np.abs(W[bk])
        return pre, gamma(K + 1) * mag + ex @ np.abs(W[wk]).T

    pre, eh = layer(x, np.zeros_like(x), "w_head", "b_head", D)
    h = np.maximum(pre, 0)
    pre, ee = layer(c, dc, "w_cos", "b_cos", N_COS)
    e = np.maximum(pre, 0)
    hh, ehh = np.repeat(h, N, axis=0), np.repeat(eh, N, axis=0)
    z = hh * e
    ez = np.abs(hh) * ee + np.abs(e) * ehh + ehh * ee + U * (np.abs(hh) + ehh) * (np.abs(e) + ee)
    pre, ey = layer(z, ez, "w_ff", "b_ff", L)
    y = np.maximum(pre, 0)
    adv, eadv = layer(y, ey, "w_adv", "b_adv", L)
    val, eval_ = layer(y, ey, "w_val", "b_val", L)
    esum = gamma(max(A - 1, 0)) * (np.abs(adv) + eadv).sum(axis=1) + eadv.sum(axis=1)
    mean = adv.mean(axis=1)
    emean = esum / A + U * (np.abs(mean) + esum / A)
    s1 = val + adv
    es1 = eval_ + eadv + U * (np.abs(s1) + eval_ + eadv)
    quant = s1 - mean[:, None]
    eq = es1 + emean[:, None] + U * (np.abs(quant) + es1 + emean[:, None])
    quant, eq = quant.reshape(B, N, A), eq.reshape(B, N, A)
    esq = gamma(max(N - 1, 0)) * (np.abs(quant) + eq).sum(axis=1) + eq.sum(axis=1)
    qv = quant.mean(axis=1)
    eqv = esq / N + U * (np.abs(qv) + esq / N)
    return quant, qv, eq, eqv


# ---------------------------------------------------------------------------------------------------------------------------- keyed taus
def keyed_taus(seed, first_env, env, agent, epoch, turn, N):
    """``[len(env), N]`` float32: u = Philox4x32-10(ctr = {(agent << 4) | (q >> 2), turn, first_env + env, epoch << 4 | 11},
    key = {seed lo, seed hi})[q & 3]; tau = (float)(u >> 8) * 2^-24."""
    env, agent = np.asarray(env, np.uint64).reshape(-1, 1), np.asarray(agent, np.uint64).reshape(-1, 1)
    q = np.arange(N, dtype=np.uint64).reshape(1, -1)
    env, agent, q = np.broadcast_arrays(env, agent, q)
    m = np.uint64(0xFFFFFFFF)
    ones = np.ones_like(env)
    w = O.philox4x32_10((agent << np.uint64(4)) | (q >> np.uint64(2)), ones * np.uint64(turn & 0xFFFFFFFF), (env + np.uint64(first_env & 0xFFFFFFFF)) & m,
                        ones * np.uint64(((epoch << 4) | STREAM_TAU) & 0xFFFFFFFF), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    sel = q & np.uint64(3)
    u = np.where(sel == 0, w[0], np.where(sel == 1, w[1], np.where(sel == 2, w[2], w[3]))).astype(np.uint64)
    return ((u >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------------- data
def random_weights(rng, D, L, A):
    """Effective weights in ``nn.Linear``'s initial ranges."""
    def uni(shape, fan):
        b = 1.0 / np.sqrt(fan)
        return rng.uniform(-b, b, size=shape).astype(F32)

    def noisy(shape, fan):
        b = np.sqrt(3.0 / fan)
        return rng.uniform(-b, b, size=shape).astype(F32)

    return dict(w_head=uni((L, D), D), b_head=uni((L,), D), w_cos=uni((L, N_COS), N_COS), b_cos=uni((L,), N_COS), w_ff=noisy((L, L), L),
                b_ff=noisy((L,), L), w_adv=noisy((A, L), L), b_adv=noisy((A,), L), w_val=noisy((L,), L), b_val=noisy((1,), L))


def effective_of(sd, train):
    """The ten effective weights of a ``state_dict`` (name -> float32 array): in training mode ``weight + sigma * epsilon`` of the noisy
    layers, every operation rounded to float32 on its own, as torch's elementwise ops do."""
    w = dict(w_head=sd["head1.weight"], b_head=sd["head1.bias"], w_cos=sd["cos_embedding.weight"], b_cos=sd["cos_embedding.bias"])
    for name, layer in (("ff", "ff_1"), ("adv", "advantage"), ("val", "value")):
        wt, bs = sd[f"{layer}.weight"], sd[f"{layer}.bias"]
        if train:
            wt = wt + sd[f"{layer}.sigma_weight"] * sd[f"{layer}.epsilon_weight"]
            bs = bs + sd[f"{layer}.sigma_bias"] * sd[f"{layer}.epsilon_bias"]
        w[f"w_{name}"], w[f"b_{name}"] = wt, bs
    w["w_val"] = w["w_val"].reshape(-1)
    return {k: np.ascontiguousarray(v, F32) for k, v in w.items()}


def load_fixture():
    """``{tag: dict}``: per set ``D, L, N, A, B``, the reference's ``state_dict`` after its train-mode call (``sd``: name -> array; the
    epsilon buffers are that call's noise), the inputs ``states`` (float32) and ``states_u8``, and per mode (``eval``, ``u8`` = eval on
    the uint8 states, ``train``) the effective weights ``w`` the reference's layers applied (recomposed from ``sd``; the generator asserted them equal to what its hooks kept), ``taus [B, N, 1]``, ``cos [B, N, 64]``,
    ``quantiles [B, N, A]``, ``qvalues [B, A]`` and the same forward in float64 (``quantiles64``).  The two large matrices of the
    reference's own shape are stored as int8 codes of a power of two (``packed``)."""
    with np.load(FIXTURE) as z:
        meta = json.loads(str(z["params"]))
        sets = {}
        for s in meta["sets"]:
            tag = s["tag"]
            d = dict(s)
            sd = {k: z[f"{tag}/sd/{k}"] for k in s["sd_keys"]}
            for k, exp in s["packed"].items():
                sd[k] = (sd[k].astype(np.float64) * 2.0 ** -exp).astype(F32)
            d["sd"] = sd
            d["states"], d["states_u8"] = z[f"{tag}/states"], z[f"{tag}/states_u8"]
            for mode in ("eval", "train", "u8"):
                d[mode] = dict(w=effective_of(sd, mode == "train"))
                for k in ("taus", "cos", "quantiles", "qvalues", "quantiles64"):
                    d[mode][k] = z[f"{tag}/{mode}/{k}"]
            sets[tag] = d
    return sets
