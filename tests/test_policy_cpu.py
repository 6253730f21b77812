"""Stochastic policies without a GPU: the NumPy restatement of ``sgw_policy_sample``'s semantics (``tests/policy_common.py``) against
what the reference's ``ActorCritic`` computed (``tests/golden/policy``) -- actions equal, log-probabilities and entropies within one
float32 ulp --, the declaration of the two entry points and the layout of ``sgw_policy_desc`` against gcc, every descriptor the call
rejects (validation precedes the launch, so no device is needed), ``RolloutBuffer.add`` with log-probabilities that already lie in the
row and under a deferred ring, and what ``ActionProbs`` / ``ActionLogits`` refuse to wrap."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from sorrel_amd import _native as N
from sorrel_amd.buffers import Buffer, RolloutBuffer
from sorrel_amd.models import ActionLogits, ActionProbs
from tests import helpers as H
from tests import learner_common as LK
from tests import policy_common as PC

META, SETS = PC.load_fixture()


# ------------------------------------------------------------------------------------------------------------- restatement against the reference
@pytest.mark.parametrize("tag", sorted(SETS))
@pytest.mark.parametrize("bits", (64, 32))
def test_restatement_reproduces_the_reference(tag, bits):
    s = SETS[tag]
    probs = s[f"probs{bits}"]
    assert probs.dtype == (np.float64 if bits == 64 else np.float32)
    u = PC.fixture_draws(META, s["idx"])
    actions, lp, ent, info = PC.restate(probs, False, u)
    assert PC.margin(info) >= PC.MARGIN and not info["bad"].any()
    assert np.array_equal(actions, s[f"actions{bits}"])
    assert (probs[np.arange(len(actions)), actions] > 0).all()                     # a zero-weight action is never chosen
    worst_lp, worst_ent = PC.ulps(lp, s[f"ref_lp{bits}"]).max(), PC.ulps(ent, s[f"ref_ent{bits}"]).max()
    print(f"{tag} float{bits}: log-prob {worst_lp} ulp, entropy {worst_ent} ulp from the reference")
    assert worst_lp <= 1 and worst_ent <= 1
    if tag != "edge":
        assert set(actions.tolist()) == set(range(probs.shape[1]))                 # the fixture exercises every action


def test_restatement_logits_invalid_rows_and_scaling():
    rng = np.random.default_rng(4)
    u = rng.integers(0, 1 << 32, size=64, dtype=np.uint64)
    p = rng.integers(1, 9, size=(64, 5)).astype(np.float64) / 1024.0
    a, lp, ent, _ = PC.restate(p, False, u)
    # logits = log of the weights give the same actions (thresholds stay clear of the sums) and, to an ulp, the same numbers
    a2, lp2, ent2, info = PC.restate(np.log(p), True, u)
    assert PC.margin(info) >= PC.MARGIN and np.array_equal(a, a2)
    assert PC.ulps(lp, lp2).max() <= 1 and PC.ulps(ent, ent2).max() <= 1
    # unnormalised weights: a power-of-two scale changes nothing at all
    a3, lp3, ent3, _ = PC.restate(p * 8.0, False, u)
    assert np.array_equal(a, a3) and np.array_equal(lp, lp3) and np.array_equal(ent, ent3)
    bad = np.array([[0.5, -0.25, 0.75], [0.5, np.nan, 0.5], [0.0, 0.0, 0.0], [np.inf, 1.0, 1.0], [0.25, 0.25, 0.5]])
    a, lp, ent, _ = PC.restate(bad, False, u[:5])
    assert a[:4].tolist() == [255] * 4 and np.isnan(lp[:4]).all() and np.isnan(ent[:4]).all() and a[4] in (0, 1, 2) and np.isfinite(lp[4])
    badl = np.array([[0.0, np.inf, 1.0], [-np.inf, -np.inf, -np.inf], [np.nan, 0.0, 0.0], [-np.inf, 0.0, -np.inf]])
    a, lp, ent, _ = PC.restate(badl, True, u[:4])
    assert a.tolist() == [255, 255, 255, 1] and lp[3] == np.float32(np.log(1 - 2.0 ** -52)) and np.isnan(lp[:3]).all()


def test_draws_are_the_oracles_counter_rng():
    from oracle import gridstep_oracle as O

    env, agent = np.array([0, 5, 5, 70000]), np.array([0, 3, 4, 127])
    u = PC.draws(0x123456789ABCDEF, 9, env, 2, 11, agent)
    for k in range(4):
        assert int(u[k]) == int(O.rng_u32(0x123456789ABCDEF, 9 + int(env[k]), 2, 11, PC.STREAM_POLICY, int(agent[k])))
    assert int(u[1]) != int(u[2])          # agents 3 and 4: another word, another counter


# ------------------------------------------------------------------------------------------------------------- header and binding
def test_header_declares_the_entry_points_and_the_binding_mirrors_them(built):
    text = open(os.path.join(H.ROOT, "include", "sgw.h")).read()
    assert re.search(r"int sgw_policy_sample\(const sgw_policy_desc\* desc, void\* stream\);", text)
    assert re.search(r"int sgw_turn_policy_sample\(sgw_engine\* eng, int32_t agent, const void\* dist, int32_t dist_type, int32_t mode, int64_t\* out_actions,\s*"
                     r"float\* log_prob_ring, float\* out_entropy, void\* stream\);", text)
    macros = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+(SGW_[A-Z_0-9]+)\s+(0x[0-9A-Fa-f]+|\d+)u?\b", text)}
    assert N.STREAM_POLICY == PC.STREAM_POLICY == 10
    streams = [v for k, v in macros.items() if k.startswith("SGW_STREAM_")]
    assert len(set(streams)) == len(streams) and max(streams) < 16             # four bits of the counter word
    assert N.load().sgw_version() == b"sgw 0.3 (gfx950)"                            # the additions are append-only
    assert PC.max_blocks() >= 2


# ------------------------------------------------------------------------------------------------------------- refusals
def good_desc():
    """A descriptor the call accepts (the pointers are never followed: every test below is rejected, or has n == 0)."""
    d = N.SgwPolicyDesc()
    d.dist = d.out_actions = d.out_log_probs = d.out_entropy = 4096
    d.n, d.num_envs, d.row_stride, d.num_actions = 0, 4, 6, 5
    d.seed, d.first_env, d.epoch, d.turn, d.agent0 = 7, 0, 1, 2, 3
    d.dist_type, d.mode = N.POLICY_F32, N.POLICY_PROBS
    return d


REJECTED = [
    ("dist is NULL", {"dist": None}, b"must not be NULL"),
    ("out_actions is NULL", {"out_actions": None}, b"must not be NULL"),
    ("n < 0", {"n": -1}, b"n ="),
    ("num_actions < 1", {"num_actions": 0}, b"num_actions"),
    ("num_actions > 256", {"num_actions": 257, "row_stride": 300}, b"num_actions"),
    ("num_envs < 1", {"num_envs": 0}, b"num_envs"),
    ("row stride below num_actions", {"row_stride": 4}, b"row_stride"),
    ("negative agent", {"agent0": -1}, b"agents"),
    ("agent0 at SGW_MAX_AGENTS", {"agent0": 128}, b"agents"),
    ("the last row's agent beyond SGW_MAX_AGENTS", {"agent0": 126, "n": 9}, b"agents"),
    ("epoch >= 2^28", {"epoch": 1 << 28}, b"epoch"),
    ("unknown dist_type", {"dist_type": 2}, b"dist_type"),
    ("negative dist_type", {"dist_type": -1}, b"dist_type"),
    ("unknown mode", {"mode": 2}, b"mode"),
    ("reserved0 set", {"reserved0": 1}, b"reserved"),
    ("reserved1 set", {"reserved1": 1}, b"reserved"),
    ("misaligned float32 dist", {"dist": 4098}, b"element type"),
    ("float64 dist on a 4-byte boundary", {"dist": 4100, "dist_type": N.POLICY_F64}, b"element type"),
    ("misaligned out_log_probs", {"out_log_probs": 4098}, b"float32"),
    ("misaligned out_entropy", {"out_entropy": 4097}, b"float32"),
    ("misaligned out_actions", {"out_actions": 4100}, b"int64"),
    ("misaligned idx", {"idx": 4100}, b"int64"),
    ("offsets past 64 bits", {"n": 1 << 40, "row_stride": 1 << 30, "idx": 4096}, b"64-bit"),
]


@pytest.mark.parametrize("case", REJECTED, ids=[c[0] for c in REJECTED])
def test_sgw_policy_sample_rejects(built, case):
    _, change, word = case
    d = good_desc()
    d.n = 5                                       # (a call that would launch, were it accepted)
    LK.assert_rejected(N.load().sgw_policy_sample, d, change, word)


def test_sgw_policy_sample_null_desc_and_no_rows(built):
    lib = N.load()
    assert lib.sgw_policy_sample(None, None) == N.EINVAL and b"desc is NULL" in lib.sgw_last_error()
    d = good_desc()
    assert lib.sgw_policy_sample(C.byref(d), None) == N.OK                       # n == 0: nothing is launched
    d.out_log_probs = d.out_entropy = None                                       # both are optional
    d.dist, d.dist_type, d.mode = 4100, N.POLICY_F32, N.POLICY_LOGITS            # float32 rows need 4-byte alignment only
    d.num_actions, d.row_stride, d.agent0 = 256, 256, 127
    assert lib.sgw_policy_sample(C.byref(d), None) == N.OK
    d.idx, d.agent0 = 4096, 500                                                  # with idx the agent keys are the device's to see
    assert lib.sgw_policy_sample(C.byref(d), None) == N.OK
    assert lib.sgw_turn_policy_sample(None, 0, 4096, 0, 0, 4096, None, None, None) == N.EINVAL and b"NULL engine" in lib.sgw_last_error()


# ------------------------------------------------------------------------------------------------------------- RolloutBuffer.add
def test_rollout_buffer_add_skips_the_copy_of_log_probs_already_in_the_row():
    buf = RolloutBuffer(3, (2,), num_envs=4, device="cpu")
    obs, rew = torch.ones(4, 2), torch.arange(4, dtype=torch.float32)
    row = buf.log_probs[0]
    row.copy_(torch.tensor([-0.5, -1.0, -1.5, -2.0]))                            # what the sampling launch wrote where it belongs
    calls = []
    real = torch.Tensor.__setitem__

    def spy(self, key, value):
        if self.data_ptr() == buf.log_probs.data_ptr():
            calls.append(key)
        return real(self, key, value)

    torch.Tensor.__setitem__ = spy
    try:
        buf.add(obs, (torch.tensor([1, 0, 1, 0]), row), rew, False)
        assert calls == []                                                       # the row itself: nothing is copied
        buf.add(obs, (torch.tensor([0, 0, 1, 1]), torch.full((4,), -0.25)), rew, False)
        assert calls == [1]                                                      # any other tensor: stored as before
        buf.add(obs, (torch.tensor([0, 0, 1, 1]), -0.75), rew, False)            # a scalar broadcasts, as before
    finally:
        torch.Tensor.__setitem__ = real
    assert buf.log_probs[0].tolist() == [-0.5, -1.0, -1.5, -2.0] and buf.log_probs[1].tolist() == [-0.25] * 4
    assert buf.log_probs[2].tolist() == [-0.75] * 4 and buf.actions[0].tolist() == [1, 0, 1, 0] and buf.idx == 0 and buf.size == 3
    # float64 log-probabilities that happen to start at the row's address are still a different tensor: converted and stored
    other = RolloutBuffer(2, (2,), num_envs=2, device="cpu")
    alias = torch.zeros(2, dtype=torch.float64)
    other.add(torch.ones(2, 2), (torch.tensor([1, 1]), alias - 3.0), torch.zeros(2), False)
    assert other.log_probs[0].tolist() == [-3.0, -3.0]


def test_rollout_buffer_add_only_counts_under_a_deferred_ring():
    buf = RolloutBuffer(3, (2,), num_envs=4, device="cpu")
    buf.log_probs.fill_(-9.0)
    buf.actions.fill_(7)
    buf._deferred = True                                                         # a recorded turn: the engine's kernels fill the rows
    buf.add(torch.ones(4, 2), (torch.tensor([1, 0, 1, 0]), torch.zeros(4)), torch.zeros(4), False)
    assert (buf.idx, buf.size, buf._deferred_adds) == (1, 1, 1)
    assert (buf.log_probs == -9.0).all() and (buf.actions == 7).all() and not buf.states.any()
    buf._deferred = False
    buf.add(torch.ones(4, 2), (torch.tensor([1, 0, 1, 0]), torch.zeros(4)), torch.zeros(4), False)
    assert buf.log_probs[1].tolist() == [0.0] * 4 and buf.actions[1].tolist() == [1, 0, 1, 0] and buf.idx == 2
    plain = Buffer(2, (2,), num_envs=4, device="cpu")                            # (an ordinary Buffer takes the actions alone, as ever)
    plain.add(torch.ones(4, 2), torch.tensor([1, 0, 1, 0]), torch.zeros(4), False)
    assert plain.actions[0].tolist() == [1, 0, 1, 0] and not hasattr(plain, "log_probs")


# ------------------------------------------------------------------------------------------------------------- the wrappers
def test_action_probs_and_logits_refuse_what_is_no_distribution():
    p = ActionProbs(torch.full((3, 4), 0.25))
    assert p.tensor.shape == (3, 4) and p.logits is False and "ActionProbs" in repr(p)
    q = ActionLogits(torch.zeros((3, 256), dtype=torch.float64))
    assert q.logits is True and isinstance(q, ActionProbs)
    for bad, err in ((torch.zeros(4), ValueError), (torch.zeros(2, 3, 4), ValueError), (torch.zeros(3, 0), ValueError), (torch.zeros(3, 257), ValueError),
                     (torch.zeros(3, 4, dtype=torch.float16), TypeError), (torch.zeros(3, 4, dtype=torch.int64), TypeError),
                     (np.zeros((3, 4), np.float32), TypeError), ([[0.5, 0.5]], TypeError)):
        for cls in (ActionProbs, ActionLogits):
            with pytest.raises(err):
                cls(bad)
