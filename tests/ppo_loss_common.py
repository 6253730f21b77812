"""What the two sgw_ppo_loss test files (and ``tools/make_ppo_loss_golden.py``) share: the NumPy restatement of the semantics stated in
``include/sgw.h`` (the distribution of ``sgw_policy_sample``, the clipped loss, torch's gradient rule), the TOLERANCES as formulas, the
reference's fixture (``tests/golden/ppo_loss/clip_loss.npz``) and small helpers.  Not collected by pytest.

Tolerances.  Every bound below is an absolute bound on the distance between two float64 evaluations of the same quantity from the same
inputs that may differ in (a) the last-bit behaviour of ``log`` / ``exp``, (b) the order of a sum, (c) a handful of correctly rounded
operations arranged differently (torch normalises the probabilities before it takes the log; autograd multiplies where the header
divides).  With ``u = 2^-53``:

* a correctly rounded operation contributes ``u`` relative; where two evaluations may arrange ``k`` such operations differently the
  term is ``2 k u`` (each side ``k u`` from the exact value);
* a sum of ``m`` terms contributes ``m u`` of the sum of the terms' magnitudes per side;
* ``log`` and ``exp`` contribute ``F`` relative per side, ``F = LIBM_ULPS * 2^-52``.  The ROCm device-library documentation installed
  with the toolchain states no bound, so ``LIBM_ULPS`` is twice the largest error measured on the MI355X against ``mpmath`` over the
  fixture's own arguments (``tools/measure_device_libm.py``; the measured figure is in DESIGN.md 0.15).

``tolerances(info)`` evaluates the formulas on the restatement's own intermediates (functions of the inputs, never of a result under
test).  Branches -- which surrogate is the minimum, whether the ratio is inside the clip range, whether a probability is clamped -- are
not covered by a tolerance: the fixture's generator asserts margins of ``2^-40`` around every one of them, and the random cases of the
GPU tests assert the same on the restatement before they compare."""
import json
import os

import numpy as np

from tests import helpers as H
from tests import learner_common as LK

FIXTURE = os.path.join(H.ROOT, "tests", "golden", "ppo_loss", "clip_loss.npz")
U = 2.0 ** -53
LIBM_ULPS = 2 * 0.57          # 2 x the largest measured error, in units of 2^-52 relative: log 0.5000, exp 0.5691 (0.5437 inside the kernel)
F = LIBM_ULPS * 2.0 ** -52
MARGIN = 2.0 ** -40           # relative distance every branch keeps from its threshold before equal branches are demanded
EPS_LO, EPS_HI = 2.0 ** -52, 1.0 - 2.0 ** -52


def max_blocks():
    return LK.max_blocks("ppo_loss.h", "kPpoMaxBlocks")


def restate(x, logits, values, actions, old, returns, eps_clip, entropy_coef, value_coef=0.5):
    """The header's arithmetic: float64, every row sum sequential in index order, every product rounded before it is added.  Returns a
    dict: per-row ``lp, H, P, d2, r, A, s1, s2, inside, gr, q, l, S, bad``, the gradients ``grad_dist [n, na]`` and ``grad_values [n]``
    (float64, before any rounding to the inputs' types) and the means ``L, Pm, M, Hm`` (``math.fsum``: the kernel's own order of the
    batch sums is not restated; the tolerance covers any order)."""
    import math

    x = np.asarray(x).astype(np.float64)
    n, na = x.shape
    v = np.asarray(values).astype(np.float64).reshape(n)
    R = np.asarray(returns).astype(np.float64).reshape(n)
    old = np.asarray(old).astype(np.float64).reshape(n)
    a = np.asarray(actions).astype(np.int64).reshape(n)
    c, vc, dn = float(entropy_coef), float(value_coef), float(n)
    lo, hi = 1.0 - float(eps_clip), 1.0 + float(eps_clip)
    with np.errstate(all="ignore"):
        bad = (a < 0) | (a >= na)
        ac = np.where(bad, 0, a)
        if logits:
            m = np.fmax.reduce(x, axis=1)
            bad |= ~(m < np.inf)
            w = np.exp(x - m[:, None])
            gaps = np.abs(x - m[:, None])
            span = float(gaps[np.isfinite(gaps)].max()) if np.isfinite(gaps).any() else 0.0
        else:
            w = x.copy()
            span = 0.0
        S = np.zeros(n)
        for i in range(na):
            S = S + w[:, i]
        bad |= ~(w >= 0.0).all(axis=1)
        bad |= ~((S > 0.0) & (S < np.inf))
        q = w / S[:, None]
        l = np.log(np.clip(q, EPS_LO, EPS_HI))
        uu = (q >= EPS_LO) & (q <= EPS_HI)
        rows = np.arange(n)
        lp = l[rows, ac]
        acc = np.zeros(n)
        for i in range(na):
            acc = acc + q[:, i] * l[:, i]
        Hrow = -acc
        r = np.exp(lp - old)
        A = R - v
        s1 = r * A
        s2 = np.clip(r, lo, hi) * A
        P = -np.minimum(s1, s2)
        d = v - R
        d2 = d * d
        inside = (r >= lo) & (r <= hi)
        half = A / 2.0
        gr = np.where(s1 < s2, A, np.where(s1 > s2, np.where(inside, A, 0.0), half + np.where(inside, half, 0.0)))
        grr = gr * r
        gl = c * q
        gl[rows, ac] = gl[rows, ac] + (-grr)
        gq = np.where(uu, gl / q, 0.0) + c * l
        t = np.zeros(n)
        for i in range(na):
            t = t + gq[:, i] * q[:, i]
        diff = gq - t[:, None]
        gd = (q * diff) / dn if logits else (diff / S[:, None]) / dn
        gv = ((2.0 * vc) * d) / dn
    for arr in (lp, Hrow, P, d2, gv):
        arr[bad] = np.nan
    gd[bad] = np.nan
    if n and not bad.any() and np.isfinite(P).all() and np.isfinite(d2).all():
        Pm, M, Hm = math.fsum(P) / dn, math.fsum(d2) / dn, math.fsum(Hrow) / dn
    else:
        Pm, M, Hm = (float(np.sum(P)) / dn, float(np.sum(d2)) / dn, float(np.sum(Hrow)) / dn) if n else (np.nan,) * 3
    L = Pm + vc * M - c * Hm
    return dict(n=n, na=na, logits=bool(logits), lp=lp, H=Hrow, P=P, d2=d2, r=r, A=A, s1=s1, s2=s2, inside=inside, gr=gr, q=q, l=l, S=S, w=w, bad=bad,
                gq=gq, t=t, span=span, grad_dist=gd, grad_values=gv, L=L, Pm=Pm, M=M, Hm=Hm, c=c, vc=vc, lo=lo, hi=hi, u=uu, a=ac)


def tolerances(info, autograd=True):
    """The formulas of the module docstring, evaluated on ``restate``'s intermediates.  Returns absolute bounds: per row ``lp, H, P, d2,
    grad_values`` and ``grad_dist [n, na]``, and scalars ``Pm, M, Hm, L``.  ``autograd=False``: neither side is torch's autograd (the
    kernel against the restatement), so the value gradient has no ``n``-term sum in it."""
    n, na, c, vc = info["n"], info["na"], abs(info["c"]), abs(info["vc"])
    q, l = info["q"], np.abs(info["l"])
    with np.errstate(all="ignore"):
        # q_i: a sum of na terms and a division, per side; for logits one exp per weight, whose argument x_i - max x is one rounding
        # (absolute u |x_i - max x|, relative in the weight)
        rel_q = 2 * ((na + 1) * U + (F + (1 + info["span"]) * U if info["logits"] else 0.0))
        # l_i = log q_i: the log's own error, relative to |l_i|, and q's relative error, absolute in the log
        tol_l = 2 * F * l + rel_q + 2 * U
        rows = np.arange(n)
        tol_lp = tol_l[rows, info["a"]]
        ql = np.abs(q) * l
        # H: na products (q's error, l's error, one rounding each) and their sum
        tol_H = (np.abs(q) * tol_l + ql * (rel_q + 2 * U)).sum(axis=1) + 2 * na * U * ql.sum(axis=1)
        # r = exp(lp - old): the argument's absolute error is a relative error of the result
        rel_r = 2 * F + tol_lp + 4 * U
        # P = -(r or its clamp) * A: A is one subtraction, the product one rounding
        tol_P = np.abs(info["r"] * info["A"]) * (rel_r + 6 * U)
        tol_d2 = 8 * U * info["d2"]
        # dL/dv: a few roundings -- and autograd's backward of the reference's BROADCAST scalar MSE adds n copies of value_coef / n
        # before it multiplies (a sum of n terms on that side; exact when n is a power of two)
        tol_gv = (8 + (n if autograd else 0)) * U * np.abs(info["grad_values"])
        # gq_i = [u_i] (c q_i - gr r [i = a]) / q_i + c l_i
        grr = np.abs(info["gr"] * info["r"])
        through = np.zeros_like(q)
        through[rows, info["a"]] = grr / q[rows, info["a"]]
        through = np.where(info["u"], through, 0.0)
        tol_gq = through * (rel_r[:, None] + rel_q + 8 * U) + c * (tol_l + 8 * U * (1.0 + l))
        mag_gqq = np.abs(info["gq"] * q)
        tol_t = (tol_gq * np.abs(q) + mag_gqq * (rel_q + 2 * U)).sum(axis=1) + 2 * na * U * mag_gqq.sum(axis=1)
        num = tol_gq + tol_t[:, None] + 2 * U * (np.abs(info["gq"]) + np.abs(info["t"])[:, None])
        scale = np.abs(q) if info["logits"] else 1.0 / info["S"][:, None]
        tol_gd = (num * scale + np.abs(info["grad_dist"]) * n * (rel_q + 8 * U)) / n
        # the means: the rows' own bounds, n terms summed (any order), one division
        def mean(tol_rows, mags):
            return (tol_rows.sum() + 2 * (n + 1) * U * np.abs(mags).sum()) / n

        tol_Pm, tol_M, tol_Hm = mean(tol_P, info["P"]), mean(tol_d2, info["d2"]), mean(tol_H, info["H"])
        tol_L = tol_Pm + vc * tol_M + c * tol_Hm + 6 * U * (abs(info["Pm"]) + vc * abs(info["M"]) + c * abs(info["Hm"]))
    return dict(lp=tol_lp, H=tol_H, P=tol_P, d2=tol_d2, grad_values=tol_gv, grad_dist=tol_gd, Pm=tol_Pm, M=tol_M, Hm=tol_Hm, L=tol_L)


def branch_margins(info, exact_ends=False):
    """The smallest relative distances from a branch, over valid rows: of the ratio from ``lo`` / ``hi``, of ``s1`` from ``s2`` outside
    the range (where they differ), and of every probability from a clamp bound (rows flagged ``exact`` by the caller excluded there)."""
    ok = ~info["bad"]
    r, s1, s2 = info["r"][ok], info["s1"][ok], info["s2"][ok]
    with np.errstate(all="ignore"):
        ratio = min(np.abs(r / info["lo"] - 1.0).min(), np.abs(r / info["hi"] - 1.0).min()) if info["lo"] > 0 else np.abs(r / info["hi"] - 1.0).min()
        out = ~info["inside"][ok] & (info["A"][ok] != 0.0)
        surr = (np.abs(s1[out] - s2[out]) / np.maximum(np.abs(s1[out]), np.abs(s2[out]))).min() if out.any() else np.inf
        q = info["q"][ok]
        near = np.minimum(np.abs(q - EPS_LO), np.abs(q - EPS_HI))
        if exact_ends:                              # a weight of exactly 0, or the only weight of its row, is clamped by every evaluation
            near = np.where((q == 0.0) | (q == 1.0), np.inf, near)
        clampd = near.min(axis=1)
    return dict(ratio=float(ratio), surrogates=float(surr), clamp_rows=clampd)


def classes(info):
    """How many valid rows fall in each of the five gradient classes."""
    r, A, lo, hi = info["r"], info["A"], info["lo"], info["hi"]
    return dict(inside=int(((r >= lo) & (r <= hi)).sum()), above_pos=int(((r > hi) & (A > 0)).sum()), above_neg=int(((r > hi) & (A < 0)).sum()),
                below_neg=int(((r < lo) & (A < 0)).sum()), below_pos=int(((r < lo) & (A > 0)).sum()))


def rounded(arr, dtype):
    """A float64 result as the kernel stores it in ``dtype``: rounded once."""
    return np.asarray(arr, np.float64).astype(dtype)


def f32_slack(arr):
    """What one rounding to float32 may add to a tolerance when the float64 value itself is only known to a tolerance: half a float32
    ulp of the value (a rounding boundary between the two float64 evaluations moves the result by one float32 step at the most, i.e.
    2^-24 relative to the next power of two above: 2^-23 of the magnitude bounds it)."""
    return np.abs(np.asarray(arr, np.float64)) * 2.0 ** -23


def load_fixture():
    """``(sets, e2e)``: ``sets[tag]`` holds ``probs, values, actions, old_log_probs, returns`` (+ ``eps_clip, entropy_coef, T, na, exact``)
    and the reference's ``loss, log_probs, entropies, grad_probs, grad_values``; ``e2e`` the end-to-end case (states, initial weights and
    the reference's parameter gradients) or None."""
    with np.load(FIXTURE) as z:
        meta = json.loads(str(z["params"]))
        sets = {}
        for m in meta["sets"]:
            tag = m["tag"]
            s = {k: z[f"{k}_{tag}"] for k in ("probs", "values", "actions", "old_log_probs", "returns", "log_probs", "entropies", "grad_probs", "grad_values")}
            s.update(loss=float(z[f"loss_{tag}"]), eps_clip=float(m["eps_clip"]), entropy_coef=float(m["entropy_coef"]), T=int(m["T"]), na=int(m["na"]),
                     exact=bool(m["exact"]))
            sets[tag] = s
        e2e = None
        if "e2e" in meta:
            e2e = dict(meta["e2e"])
            e2e.update({k[len("e2e_"):]: z[k] for k in z.files if k.startswith("e2e_")})
    return sets, e2e
