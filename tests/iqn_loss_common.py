"""What the two sgw_iqn_loss test files (and ``tools/make_iqn_loss_golden.py``) share: the NumPy restatement of the semantics stated in
``include/sgw.h`` (the double-DQN action choice, the n-step target, the pairwise TD tensor, Huber with kappa = 1, the quantile weights,
the mean and autograd's gradient with its own roundings), the kernel's ORDER of the batch sum, the TOLERANCES as formulas, the
reference's fixture (``tests/golden/iqn_loss/quantile_huber.npz``) and small helpers.  Not collected by pytest.

No libm is involved: the arithmetic is adds, multiplies, compares and ``abs``, so

* ``next_actions``, ``td_error`` and the zeros of the gradient are compared with the reference BIT FOR BIT;
* every kernel output is compared with the restatement BIT FOR BIT -- the order of every sum is part of the contract, the batch sum's
  included (``batch_sum`` below walks the kernel's tiles, threads and trees);
* the gradient against the reference's autograd, which may add the N terms of a row sum in another order and in float32:
  ``N 2^-24`` of the sum over j of ``|e_ij|``, plus ``2^-24`` of the result (the final rounding to float32);
* the loss against the reference's ``mean()``, which adds the B N N terms in torch's order: ``B N N 2^-53`` of the mean magnitude.

Branches -- which action is the maximum, which side of ``|td| = 1`` -- are not covered by a tolerance: the generator asserts margins
around every one of them outside the hand-made set, whose values are dyadic so that every order gives the same bits."""
import json
import os

import numpy as np

from tests import helpers as H
from tests import learner_common as LK
from tests.learner_common import BLOCK, bits, same_bits, tree  # noqa: F401

FIXTURE = os.path.join(H.ROOT, "tests", "golden", "iqn_loss", "quantile_huber.npz")


def max_blocks():
    return LK.max_blocks("iqn_loss.h", "kIqnMaxBlocks")


def group(N):
    """Lanes that own one batch row: the power of two at or above N."""
    g = 1
    while g < N:
        g <<= 1
    return g


def blocks_of(B, N):
    rows = BLOCK // group(N)
    return min(-(-B // rows), max_blocks())


def batch_sum(S, N):
    """The kernel's order for the sum of the row terms: a tile is 256 / G rows; workgroup k of ``blocks`` walks tiles k, k + blocks, ...;
    thread r * G of it carries row r of each tile (every other thread carries 0); a pairwise tree over the 256 threads gives the
    workgroup's partial; thread i of the merge adds partials i, i + 256, ... and the same tree merges them."""
    S = np.asarray(S, np.float64)
    B, G = S.shape[0], group(N)
    rows = BLOCK // G
    tiles = -(-B // rows)
    blocks = min(tiles, max_blocks())
    with np.errstate(all="ignore"):
        acc = np.zeros((blocks, BLOCK), np.float64)
        padded = np.zeros((-(-tiles // blocks) * blocks * rows,), np.float64)
        padded[:B] = S
        live = np.zeros(padded.shape, bool)
        live[:B] = True
        padded, live = padded.reshape(-1, blocks, rows), live.reshape(-1, blocks, rows)
        for rnd in range(padded.shape[0]):
            acc[:, ::G] = np.where(live[rnd], acc[:, ::G] + padded[rnd], acc[:, ::G])
        parts = tree(acc)
        merged = np.zeros((1, BLOCK), np.float64)
        for start in range(0, blocks, BLOCK):
            chunk = parts[start:start + BLOCK]
            merged[0, :chunk.shape[0]] = merged[0, :chunk.shape[0]] + chunk
        return float(tree(merged)[0])


def first_max(m):
    """Row-wise first maximum, a NaN counting as one (``np.argmax``'s rule, ``oracle.value_action``'s)."""
    return np.argmax(np.asarray(m, np.float32), axis=1).astype(np.int64)


def restate(q_expected, taus, q_next_local, q_next_target, actions, rewards, dones, valid, discount):
    """The header's arithmetic with the header's roundings and orders.  Returns a dict: ``next_actions [B]`` (int64), ``means [B, A]``,
    ``T [B, N]``, ``X [B, N]``, ``td_error [B, N, N]`` (float32), ``h``, ``w`` (float32 ``[B, N, N]``), ``e`` (float32), ``row_terms [B]``
    (float64), ``grad [B, N, A]`` (float32), ``grad_at_action [B, N]``, ``abs_e_sum [B, N]`` (float64: the tolerance's scale),
    ``bad [B]`` and ``L`` (float64, in the kernel's order)."""
    f32 = np.float32
    qe, ql, qt = (np.ascontiguousarray(x, f32) for x in (q_expected, q_next_local, q_next_target))
    B, N, A = qe.shape
    assert ql.shape == qt.shape == (B, N, A)
    taus = np.asarray(taus, f32).reshape(B, N)
    act = np.asarray(actions).astype(np.int64).reshape(B)
    rew, done = np.asarray(rewards, f32).reshape(B), np.asarray(dones, f32).reshape(B)
    val = np.asarray(valid).astype(np.float64).reshape(B)
    with np.errstate(all="ignore"):
        s = ql[:, 0, :].copy()
        for k in range(1, N):
            s = s + ql[:, k, :]
        means = s / f32(N)
        a_star = first_max(means) if B else np.zeros((0,), np.int64)
        bad = (act < 0) | (act >= A)
        rows = np.arange(B)
        chosen = qt[rows, :, a_star]                                               # [B, N]
        T = rew[:, None] + ((f32(discount) * chosen) * (f32(1.0) - done)[:, None])
        X = np.where(bad[:, None], f32(np.nan), qe[rows, :, np.where(bad, 0, act)])
        td = T[:, None, :] - X[:, :, None]                                         # [B, i, j]
        mag = np.abs(td)
        small = mag <= f32(1.0)
        h = np.where(small, f32(0.5) * (td * td), mag - f32(0.5)).astype(f32)
        neg = (td < 0).astype(f32)
        w = np.abs(taus[:, :, None] - neg).astype(f32)
        v3 = val[:, None, None]
        ql64 = w.astype(np.float64) * (h.astype(np.float64) * v3)
        count = float(B * N * N)
        inv = 1.0 / count if B else np.nan
        g = ((inv * w.astype(np.float64)) * v3).astype(f32)
        sg = (td > 0).astype(f32) - neg
        e = np.where(small, g * td, g * sg).astype(f32)
        sq, se, sabs = np.zeros((B, N)), np.zeros((B, N)), np.zeros((B, N))
        for j in range(N):
            sq = sq + ql64[:, :, j]
            se = se + e[:, :, j].astype(np.float64)
            sabs = sabs + np.abs(e[:, :, j].astype(np.float64))
        S = np.zeros((B,))
        for i in range(N):
            S = S + sq[:, i]
        S = np.where(bad, np.nan, S)
        gval = np.where(bad[:, None], f32(np.nan), (-se).astype(f32)).astype(f32)
        grad = np.zeros((B, N, A), f32)
        grad[rows, :, np.where(bad, 0, act)] = gval
        grad[bad] = f32(np.nan)
        L = batch_sum(S, N) / count if B else float("nan")
    return dict(B=B, N=N, A=A, next_actions=a_star, means=means, T=T, X=X, td_error=td.astype(f32), h=h, w=w, e=e, row_terms=S, grad=grad,
                grad_at_action=gval, abs_e_sum=sabs, bad=bad, L=L, ql=ql64)


def tolerances(info):
    """``grad``: ``[B, N]`` bounds for the gradient at the action taken; ``L``: the bound for the loss."""
    B, N = info["B"], info["N"]
    with np.errstate(all="ignore"):
        grad = N * 2.0 ** -24 * info["abs_e_sum"] + 2.0 ** -24 * np.abs(info["grad_at_action"].astype(np.float64))
        count = B * N * N
        L = count * 2.0 ** -53 * (np.abs(info["ql"]).sum() / max(count, 1))
    return dict(grad=grad, L=float(L))


def load_fixture():
    """``{tag: dict}``: per set the inputs (``q_expected, taus, q_next_local, q_next_target, actions, rewards, dones, valid``), ``discount``
    and the reference's ``td_error``, ``loss``, ``grad_expected`` and ``grad_next_local`` (all zero: nothing flows there)."""
    with np.load(FIXTURE) as z:
        meta = json.loads(str(z["params"]))
        sets = {}
        for s in meta["sets"]:
            d = dict(s)
            for k in ("q_expected", "taus", "q_next_local", "q_next_target", "actions", "rewards", "dones", "valid", "td_error", "loss",
                      "grad_expected", "grad_next_local"):
                d[k] = z[f"{k}_{s['tag']}"]
            sets[s["tag"]] = d
    return sets


def inputs_of(s):
    return (s["q_expected"], s["taus"], s["q_next_local"], s["q_next_target"], s["actions"], s["rewards"], s["dones"], s["valid"], s["discount"])


def random_case(rng, B, N, A, action_dtype=np.int64, valid_dtype=np.float64, weights=False):
    """Inputs in the reference's shapes: values spread so that both Huber branches and both signs occur."""
    f32 = np.float32
    qe = rng.normal(0.0, 1.5, size=(B, N, A)).astype(f32)
    ql = rng.normal(0.0, 1.5, size=(B, N, A)).astype(f32)
    qt = rng.normal(0.0, 1.5, size=(B, N, A)).astype(f32)
    taus = rng.random(size=(B, N, 1)).astype(f32)
    actions = rng.integers(0, A, size=(B, 1)).astype(action_dtype)
    rewards = (rng.integers(-4, 5, size=(B, 1)) * 0.37).astype(f32)
    dones = (rng.random(size=(B, 1)) < 0.25).astype(f32)
    valid = (rng.random(size=(B, 1)) < 0.8).astype(valid_dtype)
    if weights:
        valid = (valid * rng.random(size=(B, 1)) * 3.0).astype(valid_dtype)
    return qe, taus, ql, qt, actions, rewards, dones, valid
