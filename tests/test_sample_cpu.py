"""Replay sampling without a GPU: the declaration of ``sgw_sample`` and its ctypes mirror, every argument the call rejects (validation
precedes the launch, so no device is needed), ``TurnBuffer.sample`` on a CPU ring against a numpy restatement of the reference's
stacking, the reference's own batch (``tests/golden/replay``), and ``ReplaySampler``'s host-side range check."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from sorrel_amd import _native as N
from sorrel_amd.buffers import Buffer, ReplaySampler
from tests import helpers as H
from tests import learner_common as LK
from tests import sample_common as SC


# ------------------------------------------------------------------------------------------------------------- header and binding
def test_header_declares_sgw_sample_and_the_binding_mirrors_it(built):
    text = open(os.path.join(H.ROOT, "include", "sgw.h")).read()
    assert re.search(r"int sgw_sample\(const sgw_sample_desc\* desc, void\* stream\);", text)
    macros = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+(SGW_[A-Z_0-9]+)\s+(0x[0-9A-Fa-f]+|\d+)\b", text)}
    assert macros["SGW_STREAM_SAMPLE"] == 9 == N.STREAM_SAMPLE
    assert max(v for k, v in macros.items() if k.startswith("SGW_STREAM_")) == 9           # (the stream id lives in 4 bits)
    assert N.load().sgw_version() == b"sgw 0.3 (gfx950)"
    assert SC.max_waves() >= 64


def good_desc():
    """A descriptor the call accepts (the pointers are never followed: every test below is rejected, or has n == 0)."""
    d = N.SgwSampleDesc()
    d.states = d.actions = d.rewards = d.dones = 4096
    d.out_states = d.out_next_states = d.out_actions = d.out_rewards = d.out_dones = d.out_valid = 4096
    d.n, d.capacity, d.num_envs, d.num_starts, d.row_elems = 0, 16, 4, 10, 9
    d.state_turn_stride, d.state_env_stride, d.scalar_turn_stride, d.scalar_env_stride = 36, 9, 4, 1
    d.n_frames, d.src_type, d.act_type = 2, N.SAMPLE_F32, N.SAMPLE_ACT_I64
    return d


REJECTED = (
    [(f"{name} is NULL", {name: None}, b"must not be NULL") for name in ("states", "actions", "rewards", "dones")]
    + [(f"{name} is NULL", {name: None}, b"output") for name in ("out_states", "out_next_states", "out_actions", "out_rewards", "out_dones", "out_valid")]
    + [
        ("n < 0", {"n": -1}, b"n = -1"),
        ("n_frames < 1", {"n_frames": 0}, b"n_frames"),
        ("row_elems < 1", {"row_elems": 0}, b"row_elems"),
        ("row_elems >= 2^30", {"row_elems": 1 << 30}, b"row_elems"),
        ("num_envs < 1", {"num_envs": 0}, b"num_envs"),
        ("num_starts < 1", {"num_starts": 0}, b"num_starts"),
        ("the last row read lies outside the ring", {"num_starts": 15}, b"capacity"),
        ("num_starts >= 2^31", {"num_starts": 1 << 31, "capacity": 1 << 40}, b"num_starts"),
        ("num_envs >= 2^31", {"num_envs": 1 << 31}, b"num_envs"),
        ("starts without envs", {"starts": 4096}, b"both"),
        ("envs without starts", {"envs": 4096}, b"both"),
        ("unknown src_type", {"src_type": 2}, b"src_type"),
        ("unknown act_type", {"act_type": 2}, b"act_type"),
        ("misaligned float32 states", {"states": 4098}, b"float32"),
        ("misaligned rewards", {"rewards": 4097}, b"float32"),
        ("misaligned dones", {"dones": 4098}, b"float32"),
        ("misaligned out_states", {"out_states": 4098}, b"float32"),
        ("misaligned out_valid", {"out_valid": 4099}, b"float32"),
        ("misaligned int64 actions", {"actions": 4100}, b"int64"),
        ("misaligned starts", {"starts": 4100, "envs": 4096}, b"int64"),
        ("misaligned out_actions", {"out_actions": 4100}, b"int64"),
        ("misaligned out_index", {"out_index": 4100}, b"int64"),
        ("misaligned draw_count", {"draw_count": 4100}, b"int64"),
    ]
)


@pytest.mark.parametrize("case", REJECTED, ids=[c[0] for c in REJECTED])
def test_sgw_sample_rejects(built, case):
    _, change, word = case
    d = good_desc()
    d.n = 5                                   # (a call that would launch, were it accepted)
    LK.assert_rejected(N.load().sgw_sample, d, change, word)


def test_sgw_sample_null_desc_and_the_empty_batch(built):
    lib = N.load()
    assert lib.sgw_sample(None, None) == N.EINVAL and b"desc is NULL" in lib.sgw_last_error()
    d = good_desc()
    assert lib.sgw_sample(C.byref(d), None) == N.OK              # n == 0: nothing is launched
    d.num_starts = 14                                            # num_starts + n_frames == capacity: the last row read is the ring's last
    assert lib.sgw_sample(C.byref(d), None) == N.OK
    d.src_type, d.act_type, d.states, d.actions = N.SAMPLE_U8, N.SAMPLE_ACT_U8, 4097, 4099      # bytes need no alignment
    assert lib.sgw_sample(C.byref(d), None) == N.OK


# ------------------------------------------------------------------------------------------------------------- the CPU paths
@pytest.mark.parametrize("agent", [1, None])
@pytest.mark.parametrize("n_frames", [1, 3])
def test_turnbuffer_sample_on_a_cpu_ring(agent, n_frames):
    ring, host = SC.turn_ring(torch, "cpu", torch.uint8)
    cap, E, A = host[1].shape
    starts, envs = SC.turn_indices(cap, E * A if agent is None else E, n_frames)
    got = ring.sample(len(starts), agent=agent, n_frames=n_frames, starts=starts, envs=envs)
    want = SC.turn_expected(host, agent, n_frames, starts, envs)
    assert (want[5] == 0).any() and (want[5] == 1).any() or n_frames == 1
    SC.assert_six(got, want, f"agent={agent} n_frames={n_frames}")
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and got[3].dtype == torch.float32
    # no indices: drawn on the host, inside the ranges
    s, a, r, ns, d, v = ring.sample(7, agent=agent, n_frames=n_frames)
    assert tuple(s.shape) == (7, n_frames * 18) and tuple(a.shape) == (7, 1) and tuple(v.shape) == (7, 1)


def test_reference_batch_on_a_cpu_buffer():
    """Pins the fixture (this passes without ``sgw_sample``): the reference's history replayed into this project's Buffer, sampled at
    the reference's own draws, gives the reference's six arrays."""
    d = SC.load_fixture()
    buf = SC.replay_fixture(d, "cpu")
    got = buf.sample(len(d["draws"]), starts=d["draws"], envs=np.zeros(len(d["draws"]), np.int64))
    SC.assert_six(got, d["expected"], "reference batch")
    assert set(d["valid"].ravel().tolist()) == {0.0, 1.0} and (d["sample_dones"] == 1).any()


def test_sample_torch_is_the_cpu_path():
    d = SC.load_fixture()
    buf = SC.replay_fixture(d, "cpu")
    torch.manual_seed(5)
    a = buf.sample(8)
    torch.manual_seed(5)
    b = buf._sample_torch(8)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_replay_sampler_checks_host_index_lists():
    d = SC.load_fixture()
    buf = SC.replay_fixture(d, "cpu")
    sampler = ReplaySampler(buf, 4)
    assert sampler.n_frames == 4 and sampler.num_starts() == buf.size - 4 - 1
    hi = sampler.num_starts()
    for starts, envs in (([0, 1, hi, 2], [0, 0, 0, 0]), ([0, -1, 1, 2], [0, 0, 0, 0]), ([0, 1, 2, 3], [0, 1, 0, 0]), ([0, 1, 2, 3], [0, 0, -1, 0])):
        with pytest.raises(IndexError):
            sampler.sample(starts, envs)
    with pytest.raises(ValueError):
        sampler.sample([0, 1, 2, 3], None)
    # inside the ranges a CPU ring is read by the torch formula, into the sampler's own storage
    draws = d["draws"][:4]
    got = sampler.sample(draws, [0, 0, 0, 0])
    SC.assert_six(got, tuple(x[:4] for x in d["expected"]), "sampler on a CPU ring")
    assert np.array_equal(sampler.last_index.numpy(), np.stack([draws, np.zeros(4, np.int64)], axis=1))
    ring, _ = SC.turn_ring(torch, "cpu", torch.uint8)
    with pytest.raises(IndexError):
        ReplaySampler(ring, 2, n_frames=2, agent=None).sample([0, 1], [0, 12])          # E * A = 12 columns
    with pytest.raises(IndexError):
        ReplaySampler(ring, 2, n_frames=2, agent=0).sample([0, 1], [0, 4])              # E = 4 envs
