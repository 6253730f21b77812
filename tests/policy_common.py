"""What the two sgw_policy_sample test files share: the NumPy restatement of the semantics stated in ``include/sgw.h`` (weights, validity,
the keyed draw, the running-sum search, torch's clamped log-probability and entropy), the reference's fixture
(``tests/golden/policy/actor_critic.npz``, written by ``tools/make_policy_golden.py``), float32 ulp distances and descriptor helpers.
Not collected by pytest."""
import os

import numpy as np

from oracle import gridstep_oracle as O
from tests import helpers as H
from tests import learner_common as LK
from tests.learner_common import ulps  # noqa: F401

FIXTURE = os.path.join(H.ROOT, "tests", "golden", "policy", "actor_critic.npz")
STREAM_POLICY = 10
INVALID = 255
MARGIN = 2.0 ** -40           # share of S a threshold must keep from every running sum before equal actions are demanded of another exp / sum


def max_blocks():
    return LK.max_blocks("policy.h", "kPolicyMaxBlocks")


def draws(seed, first_env, env, epoch, turn, agent):
    """u32 of every (env, agent) pair: Philox4x32-10(ctr = {agent >> 2, turn, first_env + env, epoch << 4 | STREAM_POLICY},
    key = {seed lo, seed hi})[agent & 3] -- ``oracle.gridstep_oracle.rng_u32`` with ``index = agent``, vectorised over both."""
    env, agent = np.broadcast_arrays(np.asarray(env, np.uint64), np.asarray(agent, np.uint64))
    m = np.uint64(0xFFFFFFFF)
    ones = np.ones_like(env)
    w = O.philox4x32_10(agent >> np.uint64(2), ones * np.uint64(turn & 0xFFFFFFFF), (env + np.uint64(first_env & 0xFFFFFFFF)) & m,
                        ones * np.uint64(((epoch << 4) | STREAM_POLICY) & 0xFFFFFFFF), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    sel = agent & np.uint64(3)
    return np.where(sel == 0, w[0], np.where(sel == 1, w[1], np.where(sel == 2, w[2], w[3]))).astype(np.uint64)


def keys_of_rows(n, num_envs, agent0=0, idx=None):
    """(env, agent) of rows 0 .. n-1, as the header numbers them."""
    r = np.arange(n, dtype=np.int64) if idx is None else np.asarray(idx, np.int64)
    return r % num_envs, r // num_envs + (agent0 if idx is None else 0)


def restate(x, logits, u):
    """The header's arithmetic for rows ``x [n, num_actions]`` (float32 or float64) and draws ``u [n]``: float64, every sum sequential in
    index order, every product rounded before it is added.  Returns ``(actions int64, log_probs float32, entropy float32, info)``;
    ``info`` holds S, the running sums, the thresholds and the invalid mask."""
    x = np.asarray(x).astype(np.float64)
    n, na = x.shape
    with np.errstate(all="ignore"):
        bad = np.zeros(n, bool)
        if logits:
            m = np.fmax.reduce(x, axis=1)                      # (the maximum of the numbers; NaN only if every entry is)
            bad |= ~(m < np.inf)
            w = np.exp(x - m[:, None])
        else:
            w = x.copy()
        S, c = np.zeros(n), np.empty((n, na))
        for i in range(na):
            S = S + w[:, i]
            c[:, i] = S
        bad |= ~(w >= 0.0).all(axis=1)
        bad |= ~((S > 0.0) & (S < np.inf))
        t = (np.asarray(u).astype(np.float64) + 0.5) * 2.0 ** -32 * S
        hit = c > t[:, None]
        action = np.where(hit.any(axis=1), hit.argmax(axis=1), INVALID).astype(np.int64)
        q = w / S[:, None]
        l = np.log(np.clip(q, 2.0 ** -52, 1.0 - 2.0 ** -52))
        lp = l[np.arange(n), np.minimum(action, na - 1)]
        acc = np.zeros(n)
        for i in range(na):
            acc = acc + q[:, i] * l[:, i]
        ent = -acc
    action[bad] = INVALID
    lp[bad] = np.nan
    ent[bad] = np.nan
    return action, lp.astype(np.float32), ent.astype(np.float32), dict(S=S, c=c, t=t, bad=bad, w=w)


def margin(info):
    """The smallest distance of a row's threshold from any of its running sums, as a share of S (valid rows)."""
    ok = ~info["bad"]
    return (np.abs(info["c"][ok] - info["t"][ok, None]).min(axis=1) / info["S"][ok]).min() if ok.any() else np.inf


def load_fixture():
    """``(meta, sets)``: the keys' scalars and, per ``action_space``, a dict of probs64 / probs32 / idx / actions64 / actions32 / the
    reference's float32 log-probabilities and entropies for either input (``ref_lp64`` ...)."""
    with np.load(FIXTURE) as z:
        meta = {k: int(z[k]) for k in ("seed", "first_env", "num_envs", "epoch", "turn")}
        names = ("probs64", "probs32", "idx", "actions64", "actions32", "ref_lp64", "ref_ent64", "ref_lp32", "ref_ent32")
        sets = {str(tag): {k: z[f"{k}_{tag}"] for k in names} for tag in z["tags"]}
    return meta, sets


def fixture_draws(meta, idx):
    env, agent = keys_of_rows(len(idx), meta["num_envs"], idx=idx)
    return draws(meta["seed"], meta["first_env"], env, meta["epoch"], meta["turn"], agent)
