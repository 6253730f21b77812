"""TEST INFRASTRUCTURE ONLY -- generate ``tests/golden/replay/ring_nf4.npz`` from the reference's replay buffer.

Needs the reference checkout (``oracle/ref_loader.py``).  Usage::

    PYTHONDONTWRITEBYTECODE=1 python tools/make_replay_golden.py

What runs is the reference's own ``Buffer`` (``sorrel/buffers.py``): ``Buffer(capacity=64, obs_shape=(5, 7, 7), n_frames=4)``, 50 ``add``
calls with small-integer observations, ``done = 1`` at three turns, one ``add_empty()`` partway through, then ``np.random.seed`` and
``sample(16)``.  Stored: the history (what was added, and after which add the empty frames went in), the start rows the reference
drew (recovered from the seed: ``np.random.choice`` is called once, first thing), its six result arrays, and ``params``.  Data only: no
reference source text is stored.  The generator asserts what makes equality mean something: the batch holds samples with ``valid = 0``
and with ``valid = 1``, a sample whose own ``done`` is 1, and a sample whose frames span the empty rows."""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "replay", "ring_nf4.npz")
PARAMS = dict(capacity=64, obs_shape=[5, 7, 7], n_frames=4, adds=50, done_turns=[9, 24, 41], empty_after=30, batch=16, sample_seed=1,
              data_seed=4)


def main() -> None:
    ref_loader.install()
    from sorrel.buffers import Buffer

    P = PARAMS
    rng = np.random.default_rng(P["data_seed"])
    obs = rng.integers(0, 7, size=(P["adds"], *P["obs_shape"])).astype(np.uint8)
    actions = rng.integers(0, 5, size=P["adds"]).astype(np.int64)
    rewards = rng.integers(-10, 11, size=P["adds"]).astype(np.float32)
    dones = np.zeros(P["adds"], np.float32)
    dones[P["done_turns"]] = 1.0
    buf = Buffer(capacity=P["capacity"], obs_shape=tuple(P["obs_shape"]), n_frames=P["n_frames"])
    for i in range(P["adds"]):
        buf.add(obs[i].astype(np.float32), int(actions[i]), float(rewards[i]), float(dones[i]))
        if i == P["empty_after"]:
            buf.add_empty()
    np.random.seed(P["sample_seed"])
    states, acts, rews, next_states, dns, valid = buf.sample(P["batch"])
    np.random.seed(P["sample_seed"])
    draws = np.random.choice(max(1, buf.size - buf.n_frames - 1), P["batch"], replace=False).astype(np.int64)
    # the draws are the reference's: its first frames are those rows
    assert np.array_equal(states[:, :obs[0].size], buf.states[draws].reshape(P["batch"], -1))
    assert set(valid.ravel().tolist()) == {0.0, 1.0}, "the batch needs valid = 0 and valid = 1"
    assert (dns.ravel() == 1).any(), "the batch needs a sample whose own done is 1"
    gap = P["empty_after"] + 1
    assert ((draws <= gap) & (draws + P["n_frames"] > gap)).any(), "the batch needs a sample across the empty rows"
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, obs=obs, actions=actions, rewards=rewards, dones=dones, draws=draws,
                        states=states.astype(np.float32), sample_actions=acts.astype(np.int64), sample_rewards=rews.astype(np.float32),
                        next_states=next_states.astype(np.float32), sample_dones=dns.astype(np.float32), valid=valid.astype(np.float32),
                        idx=np.int64(buf.idx), size=np.int64(buf.size), params=json.dumps(P))
    print(f"{OUT}: {os.path.getsize(OUT)} bytes; draws = {draws.tolist()}; valid = {valid.ravel().tolist()}")


if __name__ == "__main__":
    main()
