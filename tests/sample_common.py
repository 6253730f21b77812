"""What the two replay-sampling test files share: the reference's fixture, a numpy restatement of ``sorrel/buffers.py:109-122`` (fancy
indexing on host arrays -- the expectation every comparison is made against), ring builders.  Not collected by pytest."""
import json
import os

import numpy as np

from tests import helpers as H

FIXTURE = os.path.join(H.ROOT, "tests", "golden", "replay", "ring_nf4.npz")
NAMES = ("states", "actions", "rewards", "next_states", "dones", "valid")


def max_waves():
    """The waves of the largest grid ``sgw_sample`` launches (``kSampleMaxBlocks`` workgroups of 256 threads): beyond that many
    rows the waves stride."""
    import re

    text = open(os.path.join(H.ROOT, "sorrel_amd", "csrc", "sample.h")).read()
    return int(re.search(r"kSampleMaxBlocks = (\d+);", text)[1]) * (256 // 64)


def np_sample(states, actions, rewards, dones, n_frames, starts, envs):
    """The reference's stacking over rings ``[capacity, N, ...]``: states, actions, rewards, next_states, dones, valid."""
    t0, e = np.asarray(starts, np.int64), np.asarray(envs, np.int64)
    B = len(t0)
    idx = t0[:, None] + np.arange(n_frames)
    ee = e[:, None]
    s = states[idx, ee].reshape(B, -1).astype(np.float32)
    ns = states[idx + 1, ee].reshape(B, -1).astype(np.float32)
    a = actions[idx[:, -1], e].reshape(B, -1).astype(np.int64)
    r = rewards[idx[:, -1], e].reshape(B, -1)
    d = dones[idx[:, -1], e].reshape(B, -1)
    valid = (1.0 - np.any(dones[idx[:, :-1], ee] != 0, axis=-1)).reshape(B, -1).astype(np.float32)
    return s, a, r, ns, d, valid


def load_fixture():
    with np.load(FIXTURE) as z:
        d = {k: z[k] for k in z.files}
    d["params"] = json.loads(str(d["params"]))
    d["expected"] = (d["states"], d["sample_actions"], d["sample_rewards"], d["next_states"], d["sample_dones"], d["valid"])
    return d


def replay_fixture(d, device):
    """The fixture's history through this project's ``Buffer.add`` / ``add_empty`` (one env)."""
    import torch

    from sorrel_amd.buffers import Buffer

    P = d["params"]
    buf = Buffer(P["capacity"], tuple(P["obs_shape"]), n_frames=P["n_frames"], num_envs=1, device=device)
    for i in range(P["adds"]):
        buf.add(torch.from_numpy(d["obs"][i].astype(np.float32))[None].to(device), torch.tensor([int(d["actions"][i])], device=device),
                torch.tensor([float(d["rewards"][i])], device=device), bool(d["dones"][i]))
        if i == P["empty_after"]:
            buf.add_empty()
    assert buf.idx == int(d["idx"]) and buf.size == int(d["size"])
    return buf


def assert_six(got, want, ctx=""):
    for name, g, w in zip(NAMES, got, want):
        g = g.detach().cpu().numpy() if hasattr(g, "detach") else np.asarray(g)
        assert g.shape == tuple(np.asarray(w).shape), f"{ctx}: {name} has shape {g.shape}, expected {np.asarray(w).shape}"
        assert np.array_equal(g, w), f"{ctx}: {name} differs"


def turn_ring(torch, device, obs_dtype, seed=3, A=3, E=4, capacity=12, window=(2, 3, 3)):
    """A filled ``TurnBuffer`` (observations over every byte value, dones set in two slots) and host copies of its arrays."""
    from sorrel_amd.buffers import TurnBuffer

    rng = np.random.default_rng(seed)
    ring = TurnBuffer(capacity, E, (A, *window), device=device, obs_dtype=obs_dtype)
    obs = rng.integers(0, 256, size=(capacity, E, A, *window)).astype(np.uint8)
    obs.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)                     # every byte value, whatever the draw
    act = rng.integers(0, 250, size=(capacity, E, A)).astype(np.uint8)
    rew = rng.integers(-9, 10, size=(capacity, E, A)).astype(np.float32)
    don = np.zeros((capacity, E, A), np.float32)
    don[4, 1, :] = 1.0
    don[7, :, 1] = 1.0
    ring.obs.copy_(torch.from_numpy(obs).to(ring.obs.dtype))
    ring.actions.copy_(torch.from_numpy(act))
    ring.rewards.copy_(torch.from_numpy(rew))
    ring.dones.copy_(torch.from_numpy(don))
    ring.advance(capacity)
    return ring, (obs, act, rew, don)


def turn_expected(host, agent, n_frames, starts, envs):
    obs, act, rew, don = host
    cap, E, A = act.shape
    if agent is None:
        return np_sample(obs.reshape(cap, E * A, -1), act.reshape(cap, E * A), rew.reshape(cap, E * A), don.reshape(cap, E * A),
                         n_frames, starts, envs)
    return np_sample(obs[:, :, agent].reshape(cap, E, -1), act[:, :, agent], rew[:, :, agent], don[:, :, agent], n_frames, starts, envs)


def turn_indices(cap, cols, n_frames, n=23, seed=9):
    """Starts and columns that include both ends of both ranges, and repeats."""
    rng = np.random.default_rng(seed + n_frames)
    hi = cap - n_frames - 1
    starts = rng.integers(0, hi, size=n)
    envs = rng.integers(0, cols, size=n)
    starts[:4] = (0, hi - 1, 0, hi - 1)
    envs[:4] = (0, cols - 1, cols - 1, 0)
    starts[5], envs[5] = starts[4], envs[4]
    return starts.astype(np.int64), envs.astype(np.int64)
