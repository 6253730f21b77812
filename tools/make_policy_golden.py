"""TEST INFRASTRUCTURE ONLY -- generate ``tests/golden/policy/actor_critic.npz`` from the reference's PPO actor.

Needs the reference checkout (``oracle/ref_loader.py``).  Usage::

    PYTHONDONTWRITEBYTECODE=1 python tools/make_policy_golden.py

Hand-made states go through the reference's own ``ActorCritic`` (``sorrel/models/pytorch/ppo.py:68-158``, ``layer_size`` 4) for
``action_space`` 2 / 3 / 4 / 5 / 9 / 17.  Stored per action space ``n`` (data only):

* ``probs64_n`` the actor's float64 probabilities, ``probs32_n`` their float32 cast;
* ``idx_n`` the rows' keys ``agent * num_envs + env`` (with the scalars ``seed``, ``first_env``, ``num_envs``, ``epoch``, ``turn``);
* ``actions64_n`` / ``actions32_n``: the action the rule of ``include/sgw.h`` picks from either -- ``t = (u + 0.5) 2^-32 S``, the first
  running sum above ``t`` -- with ``u`` from ``oracle.gridstep_oracle.rng_u32`` (stream 10, index = agent), in plain Python floats;
* ``ref_lp64_n`` / ``ref_ent64_n``: the reference's ``evaluate(state, action)`` log-probabilities and entropies, cast to float32;
  ``ref_lp32_n`` / ``ref_ent32_n``: the same two quantities of ``torch.distributions.Categorical`` -- the class ``evaluate`` builds --
  over the float32 cast taken to float64 (the actor itself never emits float32).

The set ``edge`` holds hand-made rows of 4 actions with exact zeros and rows with one action at probability 1 (``Categorical`` directly).

The generator asserts what makes the fixture mean something: every action of every space is chosen somewhere; over 65 536 keyed draws
from one fixed row every action's count lies within 6 binomial standard deviations of ``n q_i`` (the draws are deterministic: this holds
or the rule is wrong); no row's threshold lies closer than ``2^-40 S`` to a running sum."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_loader  # noqa: E402
from oracle.gridstep_oracle import rng_u32  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "policy", "actor_critic.npz")
SPACES = (2, 3, 4, 5, 9, 17)
ROWS, INPUTS = 160, 6
STREAM_POLICY = 10
SEED, FIRST_ENV, NUM_ENVS, EPOCH, TURN = 0x5EED0123456789AB, 1000, 8, 3, 7
MAX_AGENTS = 128


def states_of(n_actions: int) -> np.ndarray:
    """Hand-made: small integers in a fixed pattern, scaled so that the actor's tanh layers leave their linear range."""
    r = np.arange(ROWS)[:, None]
    c = np.arange(INPUTS)[None, :]
    return (((r * (2 * c + 3) + n_actions * c * c + r * r // 7) % 17) - 8).astype(np.float64) * 0.75


def pick(row, u):
    """(action, smallest |c_i - t| / S) by the rule of include/sgw.h, in Python floats (float64), sequentially."""
    w = [float(v) for v in row]
    S = 0.0
    for v in w:
        S += v
    t = (float(u) + 0.5) * 2.0 ** -32 * S
    c, action, gap = 0.0, None, float("inf")
    for i, v in enumerate(w):
        c += v
        gap = min(gap, abs(c - t) / S)
        if action is None and c > t:
            action = i
    assert action is not None and w[action] > 0.0
    return action, gap


def draw(idx):
    env, agent = int(idx) % NUM_ENVS, int(idx) // NUM_ENVS
    return int(rng_u32(SEED, FIRST_ENV + env, EPOCH, TURN, STREAM_POLICY, agent))


def main() -> None:
    ref_loader.install()
    import torch
    from torch.distributions import Categorical

    from sorrel.models.pytorch import ppo

    arrays, tags = {}, []
    rng = np.random.default_rng(20)

    def store(tag, probs64, lp64_ent64=None):
        n_rows, na = probs64.shape
        probs32 = probs64.astype(np.float32)
        idx = rng.integers(0, NUM_ENVS * MAX_AGENTS, size=n_rows).astype(np.int64)
        us = [draw(i) for i in idx]
        a64, a32, gap = [], [], float("inf")
        for k in range(n_rows):
            a, g = pick(probs64[k], us[k])
            a64.append(a)
            gap = min(gap, g)
            a, g = pick(probs32[k], us[k])
            a32.append(a)
            gap = min(gap, g)
        assert gap >= 2.0 ** -40, f"{tag}: a threshold lies {gap:.3e} S from a running sum"
        a64, a32 = np.asarray(a64, np.int64), np.asarray(a32, np.int64)
        if lp64_ent64 is None:
            d = Categorical(torch.tensor(probs64))
            lp64, ent64 = d.log_prob(torch.tensor(a64)), d.entropy()
        else:
            lp64, ent64 = lp64_ent64(a64)
        d32 = Categorical(torch.tensor(probs32).double())
        lp32, ent32 = d32.log_prob(torch.tensor(a32)), d32.entropy()
        arrays.update({f"probs64_{tag}": probs64, f"probs32_{tag}": probs32, f"idx_{tag}": idx, f"actions64_{tag}": a64, f"actions32_{tag}": a32,
                       f"ref_lp64_{tag}": lp64.detach().numpy().astype(np.float32), f"ref_ent64_{tag}": ent64.detach().numpy().astype(np.float32),
                       f"ref_lp32_{tag}": lp32.numpy().astype(np.float32), f"ref_ent32_{tag}": ent32.numpy().astype(np.float32)})
        tags.append(str(tag))
        return a64, a32, gap

    for na in SPACES:
        torch.manual_seed(100 + na)
        ac = ppo.ActorCritic(input_size=INPUTS, action_space=na, layer_size=4)
        with torch.no_grad():
            for layer in ac.actor:                       # (the default initialisation leaves the softmax nearly uniform: spread it)
                if isinstance(layer, torch.nn.Linear):
                    layer.weight.mul_(2.5)
        states = torch.tensor(states_of(na))
        with torch.no_grad():
            probs64 = ac.actor(states).numpy().copy()
        assert probs64.dtype == np.float64 and probs64.shape == (ROWS, na)

        def evaluate(actions, ac=ac, states=states):
            with torch.no_grad():
                lp, _values, ent = ac.evaluate(states, torch.tensor(actions))
            return lp, ent

        a64, a32, gap = store(na, probs64, evaluate)
        for name, acts in (("float64", a64), ("float32", a32)):
            assert set(acts.tolist()) == set(range(na)), f"action_space {na} ({name}): actions {sorted(set(range(na)) - set(acts.tolist()))} are never chosen"
        # 65 536 keyed draws from row 0: 512 (env, turn) pairs x 128 agents
        counts = np.zeros(na, np.int64)
        for j in range(512):
            us = rng_u32(SEED, FIRST_ENV + j % 64, EPOCH, 1 + j // 64, STREAM_POLICY, np.arange(MAX_AGENTS))
            for u in us:
                counts[pick(probs64[0], int(u))[0]] += 1
        n = 512 * MAX_AGENTS
        q = probs64[0] / probs64[0].sum()
        sd = np.sqrt(n * q * (1 - q))
        assert (np.abs(counts - n * q) <= 6 * sd).all(), f"action_space {na}: counts {counts} against expected {n * q}"
        print(f"action_space {na}: {ROWS} rows, min gap {gap:.3e} S, worst count deviation {np.abs(counts - n * q).max() / sd.max():.2f} sd")

    edge = np.array([[0.0, 0.5, 0.5, 0.0], [0.25, 0.0, 0.0, 0.75], [0.0, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0],
                     [0.0, 0.125, 0.0, 0.875], [0.5, 0.0, 0.5, 0.0], [0.0, 1.0, 0.0, 0.0]] * 4, np.float64)
    a64, _a32, gap = store("edge", edge)
    assert all(edge[k, a] > 0 for k, a in enumerate(a64))
    print(f"edge rows: {len(edge)}, min gap {gap:.3e} S")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, tags=np.array(tags), seed=np.uint64(SEED), first_env=np.int64(FIRST_ENV), num_envs=np.int64(NUM_ENVS),
                        epoch=np.int64(EPOCH), turn=np.int64(TURN), **arrays)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
