"""What the two sgw_iqn_backward test files (and ``tools/make_iqn_backward_golden.py``) share: the NumPy restatement of the semantics stated
in ``include/sgw.h`` (every dot product and every reduction ONE fused multiply-add chain in ascending index order that starts at +0; the
forward's own chains start at the bias), the CAP against the reference as a formula, and the reference's fixture
(``tests/golden/iqn_backward/backward.npz``).  Not collected by pytest.

* Every kernel output is compared with the restatement BIT FOR BIT, fed the kernel's own cos (``cosf`` is the one library call).
* Against the reference (torch's autograd on the CPU, which sums in its own order), per parameter tensor: ``d_ref`` = max |reference
  float32 - float64|, ``d`` = the same for the side under test; the cap is ``d <= 4 d_ref + 2^-22 max|g64|``.  Both sides are float32
  evaluations of the same sums in different orders; a wrong or missing term shows at relative order 1 / K, far above a factor of 4."""
import json
import os

import numpy as np

from tests import helpers as H
from tests import iqn_forward_common as FC

FIXTURE = os.path.join(H.ROOT, "tests", "golden", "iqn_backward", "backward.npz")
F32 = np.float32
WEIGHTS = FC.WEIGHTS
# the parameter a gradient of an effective weight belongs to, and the noisy layers' (sigma, epsilon)
PARAM = dict(w_head="head1.weight", b_head="head1.bias", w_cos="cos_embedding.weight", b_cos="cos_embedding.bias", w_ff="ff_1.weight",
             b_ff="ff_1.bias", w_adv="advantage.weight", b_adv="advantage.bias", w_val="value.weight", b_val="value.bias")
NOISY = dict(w_ff=("ff_1.sigma_weight", "ff_1.epsilon_weight"), b_ff=("ff_1.sigma_bias", "ff_1.epsilon_bias"),
             w_adv=("advantage.sigma_weight", "advantage.epsilon_weight"), b_adv=("advantage.sigma_bias", "advantage.epsilon_bias"),
             w_val=("value.sigma_weight", "value.epsilon_weight"), b_val=("value.sigma_bias", "value.epsilon_bias"))
SMALL_SETS = FC.SETS[:3]
BIG_TAG = "875_250_12_4_8"
BIG_HEAD_ROWS = slice(0, None, 8)             # the rows of head1.weight's gradient the fixture keeps of the reference's own shape


def mask(x):
    """``!(x <= 0)``: torch's ``threshold_backward`` -- 0 at 0, a NaN passes the gradient."""
    with np.errstate(invalid="ignore"):
        return ~(np.asarray(x) <= 0)


def chain_rows(x, w):
    """``[M, K] , [K, J] -> [M, J]``: element (m, j) is fmaf(x_K-1, w[K-1][j], ... fmaf(x_0, w[0][j], +0))."""
    x, w = np.asarray(x, F32), np.asarray(w, F32)
    acc = np.zeros((x.shape[0], w.shape[1]), F32)
    for k in range(x.shape[1]):
        acc = FC.fmaf(x[:, k, None], w[None, k, :], acc)
    return acc


def chain_batch(g, act):
    """``[M, J] , [M, K] -> [J, K]``: element (j, k) is the chain over the batch rows m ascending of ``g[m][j] * act[m][k]``, from +0."""
    g, act = np.asarray(g, F32), np.asarray(act, F32)
    acc = np.zeros((g.shape[1], act.shape[1]), F32)
    for m in range(g.shape[0]):
        acc = FC.fmaf(g[m, :, None], act[m, None, :], acc)
    return acc


def serial_sum(x, axis):
    """``((x_0 + x_1) + ...)`` along ``axis`` in float32."""
    x = np.moveaxis(np.asarray(x, F32), axis, 0)
    s = x[0].copy()
    for i in range(1, x.shape[0]):
        s = (s + x[i]).astype(F32)
    return s


def restate(w, states, cos, grad):
    """The header's arithmetic behind ``cos`` (float32 ``[B, N, 64]``) for ``grad`` = dL/dquantiles ``[B, N, A]``: a dict of the ten
    gradients by the names of ``WEIGHTS`` (each in its weight's shape) and ``grad_h [B, L]``."""
    x = np.asarray(states).astype(F32)
    cos = np.asarray(cos, F32)
    B, N = cos.shape[0], cos.shape[1]
    A, L = np.asarray(w["w_adv"]).shape[0], np.asarray(w["w_ff"]).shape[0]
    M = B * N
    c = cos.reshape(M, FC.N_COS)
    g = np.asarray(grad, F32).reshape(M, A)
    ones = np.ones((M, 1), F32)
    with np.errstate(all="ignore"):
        h = FC.relu(FC.chain(x, w["w_head"], w["b_head"]))
        e = FC.relu(FC.chain(c, w["w_cos"], w["b_cos"]))
        hm = np.repeat(h, N, axis=0)
        z = (hm * e).astype(F32)
        y = FC.relu(FC.chain(z, w["w_ff"], w["b_ff"]))
        G = serial_sum(g, 1)
        dO = np.concatenate([(g - (G / F32(A)).astype(F32)[:, None]).astype(F32), G[:, None]], axis=1)
        Wo = np.concatenate([np.asarray(w["w_adv"], F32), np.asarray(w["w_val"], F32).reshape(1, L)], axis=0)
        dy = np.where(mask(y), chain_rows(dO, Wo), F32(0.0)).astype(F32)
        dz = chain_rows(dy, w["w_ff"])
        de = np.where(mask(e), (dz * hm).astype(F32), F32(0.0)).astype(F32)
        dh = serial_sum((dz * e).astype(F32).reshape(B, N, L), 1)
        dhp = np.where(mask(h), dh, F32(0.0)).astype(F32)
        out = dict(grad_h=dh)
        for name, gm, act in (("adv", dO[:, :A], y), ("val", dO[:, A:], y), ("ff", dy, z), ("cos", de, c), ("head", dhp, x)):
            both = chain_batch(gm, np.concatenate([act, ones[:act.shape[0]]], axis=1))
            out["w_" + name], out["b_" + name] = both[:, :-1].copy(), both[:, -1].copy()
        out["w_val"] = out["w_val"].reshape(np.asarray(w["w_val"]).shape)
    return out


def parameter_grads(gw, sd, train):
    """The gradients of a module's parameters from those of its ten effective weights: the weights' own, and in training mode
    ``sigma``'s = ``g * epsilon`` (float32, as torch's elementwise backward of ``weight + sigma * epsilon`` forms it)."""
    out = {}
    for name in WEIGHTS:
        g = np.asarray(gw[name], F32)
        out[PARAM[name]] = g.reshape(np.asarray(sd[PARAM[name]]).shape)
        if train and name in NOISY:
            sigma, eps = NOISY[name]
            out[sigma] = (g.reshape(np.asarray(sd[eps]).shape) * np.asarray(sd[eps], F32)).astype(F32)
    return out


def cap(d_ref, g64):
    """``4 d_ref + 2^-22 max|g64|``"""
    g64 = np.asarray(g64, np.float64)
    return 4.0 * float(d_ref) + 2.0 ** -22 * (float(np.abs(g64).max()) if g64.size else 0.0)


def distance(g, g64):
    g, g64 = np.asarray(g, np.float64), np.asarray(g64, np.float64)
    return float(np.abs(g.reshape(g64.shape) - g64).max()) if g64.size else 0.0


def load_fixture():
    """``{case: dict}``.  The small cases (``<D>_<L>_<N>_<A>_<B>/eval`` and ``/train``): ``sd`` (the reference's ``state_dict`` after the
    call: its epsilon buffers are that call's noise), ``train``, ``states``, ``taus [B, N, 1]``, ``cos``, ``grad`` (dL/dquantiles),
    ``g32`` and ``g64`` (name -> autograd's gradients of every parameter in float32, and of a float64 copy of the module), ``d_ref`` and
    ``d_r`` (name -> the two distances the generator found).  The case of the reference's own shape (``BIG_TAG``) takes weights, states,
    taus and cos from the forward's fixture and stores ``grad``, ``g64`` rounded to float32 (``head1.weight``: ``BIG_HEAD_ROWS``) and
    ``d_ref``."""
    fwd = FC.load_fixture()
    with np.load(FIXTURE) as z:
        meta = json.loads(str(z["params"]))
        cases = {}
        for c in meta["cases"]:
            tag = c["case"]
            d = dict(c)
            if c["big"]:
                s = fwd[c["set"]]
                d["sd"], d["states"], d["taus"], d["cos"] = s["sd"], s["states"], s["eval"]["taus"], s["eval"]["cos"]
            else:
                d["sd"] = {k: z[f"{tag}/sd/{k}"] for k in c["sd_keys"]}
                d["states"], d["taus"], d["cos"] = z[f"{tag}/states"], z[f"{tag}/taus"], z[f"{tag}/cos"]
                d["g32"] = {k: z[f"{tag}/g32/{k}"] for k in c["grad_keys"]}
            d["grad"] = z[f"{tag}/grad"]
            d["g64"] = {k: z[f"{tag}/g64/{k}"] for k in c["grad_keys"]}
            cases[tag] = d
    return cases


def kept(name, g, case):
    """The part of parameter ``name``'s gradient the fixture holds of ``case``."""
    return g[BIG_HEAD_ROWS] if case["big"] and name == "head1.weight" else g
