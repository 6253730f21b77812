"""IQN's quantile Huber loss without a GPU: the NumPy restatement of ``sgw_iqn_loss``'s semantics (``tests/iqn_loss_common.py``) against what
the reference's ``iRainbowModel.train_step`` computed (``tests/golden/iqn_loss``) -- ``td_error`` and the gradient's zeros bit for bit, the
gradient and the loss each within its tolerance FORMULA --, ties, NaNs and an out-of-range action, the declaration of the entry points
and the layout of ``sgw_iqn_loss_desc`` against gcc, every descriptor the call rejects (validation precedes the launch, so no device is
needed), ``_iqn_loss_torch`` against the fixture, what the Python wrappers refuse, and ``iqn_loss`` on CPU tensors backpropagating to a
leaf."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from sorrel_amd import _native as N
from sorrel_amd import compat, losses
from tests import helpers as H
from tests import learner_common as LK
from tests import iqn_loss_common as LC

SETS = LC.load_fixture()


def within(got, want, tol, what, ctx):
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    share = float(np.max(err / np.maximum(tol, 1e-300))) if np.size(err) else 0.0
    print(f"{ctx} {what}: {share:.4f} of the tolerance")
    assert share <= 1.0, (ctx, what, share)


def at_action(grad, actions):
    B = grad.shape[0]
    return grad[np.arange(B), :, np.asarray(actions).reshape(B)]


def off_action(grad, actions):
    B = grad.shape[0]
    mask = np.ones(grad.shape, bool)
    mask[np.arange(B), :, np.asarray(actions).reshape(B)] = False
    return grad[mask]


def tensors(s, device="cpu"):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(device) for x in LC.inputs_of(s)[:8]) + (s["discount"],)


# ------------------------------------------------------------------------------------------------------------- restatement against the reference
def test_the_fixture_covers_what_the_issue_lists():
    assert {s["A"] for s in SETS.values()} >= {2, 3, 4, 5, 9, 17}
    assert {s["N"] for s in SETS.values()} >= {1, 2, 8, 12, 13, 64}
    assert {s["B"] for s in SETS.values()} >= {1, 2, 37, 64}
    assert sum(s["exact"] for s in SETS.values()) == 1
    assert os.path.getsize(LC.FIXTURE) < 512 * 1024
    for s in SETS.values():
        assert s["valid"].dtype == np.float64 and s["actions"].dtype == np.int64 and s["valid"].shape == (s["B"], 1)
        assert not s["grad_next_local"].any() and s["next_local_grad_absent"]


@pytest.mark.parametrize("tag", sorted(SETS))
def test_restatement_reproduces_the_reference(tag):
    s = SETS[tag]
    info = LC.restate(*LC.inputs_of(s))
    assert not info["bad"].any() and (info["B"], info["N"], info["A"]) == (s["B"], s["N"], s["A"])
    LC.same_bits(info["td_error"], s["td_error"], "td_error", tag)
    LC.same_bits(off_action(s["grad_expected"], s["actions"]), off_action(info["grad"], s["actions"]), "the gradient's zeros", tag)
    assert not LC.bits(off_action(info["grad"], s["actions"])).any()                  # exact +0
    tol = LC.tolerances(info)
    within(at_action(s["grad_expected"], s["actions"]), info["grad_at_action"], tol["grad"], "dL/dq_expected", tag)
    within(s["loss"], info["L"], tol["L"], "loss", tag)
    if s["B"] >= 32:
        mag = np.abs(info["td_error"])
        assert (mag <= 1).any() and (mag > 1).any() and (info["td_error"] < 0).any() and (info["td_error"] > 0).any()
        assert np.abs(s["grad_expected"]).max() > 1e-5 and s["loss"] > 1e-3           # (the bounds are not met by zeros)
    if s["exact"]:
        assert (info["td_error"] == 0).any() and (np.abs(info["td_error"]) == 1).any()
        top = np.sort(info["means"], axis=1)
        assert (top[:, -1] == top[:, -2]).any()
        assert np.array_equal(info["grad"], s["grad_expected"]) and info["L"] == float(s["loss"])
    assert np.array_equal(info["row_terms"], info["ql"].sum(axis=(1, 2))) or np.allclose(info["row_terms"], info["ql"].sum(axis=(1, 2)), rtol=1e-13, atol=0)


def test_restatement_ties_nan_and_an_out_of_range_action():
    rng = np.random.default_rng(7)
    B, Nq, A = 6, 3, 5
    qe, taus, ql, qt, actions, rewards, dones, valid = LC.random_case(rng, B, Nq, A)
    ql[:] = 0.25
    ql[0, :, 3] = 0.5
    ql[0, :, 1] = 0.5                                   # a tie: the first maximum
    ql[1, 1, 4] = np.nan
    ql[1, 0, 2] = np.nan                                # two NaN means: the first NaN
    ql[2, :, 0] = np.inf
    ql[2, 2, 3] = np.nan                                # a NaN beats +inf
    ql[3, :, 4] = -0.0
    ql[3, :, :4] = 0.0                                  # -0 == +0: the first
    actions[4, 0] = A                                   # out of range
    info = LC.restate(qe, taus, ql, qt, actions, rewards, dones, valid, 0.9)
    assert info["next_actions"].tolist()[:4] == [1, 2, 3, 0] and info["next_actions"][4] == 0 and info["next_actions"][5] == 0
    assert info["bad"].tolist() == [False] * 4 + [True, False]
    assert np.isnan(info["grad"][4]).all() and np.isnan(info["row_terms"][4]) and np.isnan(info["td_error"][4]).all() and np.isnan(info["L"])
    assert not np.isnan(info["grad"][[0, 1, 2, 3, 5]]).any() and not np.isnan(info["row_terms"][[0, 1, 2, 3, 5]]).any()
    actions[4, 0] = -1
    assert LC.restate(qe, taus, ql, qt, actions, rewards, dones, valid, 0.9)["bad"][4]
    # the batch sum walks the kernel's tiles: more rows than one launch holds in a single round, and a size no tile divides
    S = rng.random(size=(LC.max_blocks() * 128 + 131,))
    assert abs(LC.batch_sum(S, 2) - S.sum()) <= 1e-9 * S.sum() and LC.batch_sum(S[:5], 64) == float(((((S[0] + S[1]) + (S[2] + S[3])) + S[4])))


# ------------------------------------------------------------------------------------------------------------- header and binding
def test_header_declares_the_entry_points_and_the_binding_mirrors_them(built):
    text = open(os.path.join(H.ROOT, "include", "sgw.h")).read()
    assert re.search(r"int sgw_iqn_loss\(const sgw_iqn_loss_desc\* desc, void\* stream\);", text)
    assert re.search(r"int64_t sgw_iqn_loss_workspace_bytes\(int64_t n, int32_t num_quantiles\);", text)
    assert N.IQN_MAX_QUANTILES == 64
    lib = N.load()
    assert lib.sgw_version() == b"sgw 0.3 (gfx950)"                            # the additions are append-only
    blocks = LC.max_blocks()
    assert blocks >= 2
    wb = lib.sgw_iqn_loss_workspace_bytes
    assert wb(0, 12) == 0 and wb(1, 12) == 8 and wb(16, 12) == 8 and wb(17, 12) == 16 and wb(5, 64) == 16 and wb(257, 1) == 16
    assert wb(1 << 40, 12) == blocks * 8
    assert [wb(b, n) for b, n in ((64, 12), (65, 33), (257, 2))] == [LC.blocks_of(b, n) * 8 for b, n in ((64, 12), (65, 33), (257, 2))]
    assert wb(-1, 12) == N.EINVAL and b"n =" in lib.sgw_last_error()
    assert wb(4, 0) == N.EINVAL and wb(4, 65) == N.EINVAL and b"num_quantiles" in lib.sgw_last_error()
    assert wb((1 << 63) - 1, 1) == N.EINVAL and wb(1 << 58, 64) == N.EINVAL                 # (no overflow)
    assert "models.pytorch" in compat.OUT_OF_SCOPE and "iqn_loss" in compat.OUT_OF_SCOPE["models.pytorch"]


# ------------------------------------------------------------------------------------------------------------- refusals
INPUTS = ("q_next_local", "q_next_target", "q_expected", "taus", "actions", "rewards", "dones", "valid")


def good_desc():
    """A descriptor the call accepts (the pointers are never followed: every test below is rejected, or has n == 0)."""
    d = N.SgwIqnLossDesc()
    for name in INPUTS:
        setattr(d, name, 4096)
    d.out_terms = d.out_grad_expected = d.out_next_actions = d.out_row_terms = d.out_td_error = d.workspace = 8192
    d.workspace_bytes = 1 << 20
    d.n, d.num_quantiles, d.num_actions, d.discount = 0, 12, 5, 0.97
    d.action_type, d.valid_type = N.PPO_ACT_I64, N.POLICY_F32
    return d


REJECTED = [(f"{name} is NULL", {name: None}, b"must not be NULL") for name in INPUTS + ("out_terms",)] + [
    ("n < 0", {"n": -1}, b"n ="),
    ("num_quantiles < 1", {"num_quantiles": 0}, b"num_quantiles"),
    ("num_quantiles > 64", {"num_quantiles": 65}, b"num_quantiles"),
    ("num_actions < 1", {"num_actions": 0}, b"num_actions"),
    ("num_actions > 256", {"num_actions": 257}, b"num_actions"),
    ("unknown action_type", {"action_type": 2}, b"action_type"),
    ("negative action_type", {"action_type": -1}, b"action_type"),
    ("unknown valid_type", {"valid_type": 2}, b"valid_type"),
    ("negative valid_type", {"valid_type": -1}, b"valid_type"),
    ("reserved0 set", {"reserved0": 1}, b"reserved"),
    ("reserved1 set", {"reserved1": 1}, b"reserved"),
    ("infinite discount", {"discount": float("inf")}, b"discount"),
    ("negative infinite discount", {"discount": float("-inf")}, b"discount"),
    ("NaN discount", {"discount": float("nan")}, b"discount"),
] + [(f"misaligned {name}", {name: 4098}, b"float32") for name in ("q_next_local", "q_next_target", "q_expected", "taus", "rewards", "dones")] + [
    ("misaligned out_grad_expected", {"out_grad_expected": 8194}, b"float32"),
    ("misaligned out_td_error", {"out_td_error": 8193}, b"float32"),
    ("misaligned int64 actions", {"actions": 4100}, b"actions"),
    ("misaligned float32 valid", {"valid": 4098}, b"valid"),
    ("float64 valid on a 4-byte boundary", {"valid": 4100, "valid_type": N.POLICY_F64}, b"valid"),
    ("misaligned out_terms", {"out_terms": 8196}, b"8-byte"),
    ("misaligned out_next_actions", {"out_next_actions": 8196}, b"8-byte"),
    ("misaligned out_row_terms", {"out_row_terms": 8196}, b"8-byte"),
    ("misaligned workspace", {"workspace": 8196}, b"8-byte"),
    ("no workspace", {"workspace": None}, b"workspace"),
    ("a workspace that is too small", {"workspace_bytes": 7}, b"workspace"),
    ("a workspace too small for two tiles", {"n": 17, "workspace_bytes": 15}, b"workspace"),
    ("offsets past 64 bits", {"n": 1 << 50, "num_quantiles": 64, "num_actions": 256}, b"64-bit"),
]


@pytest.mark.parametrize("case", REJECTED, ids=[c[0] for c in REJECTED])
def test_sgw_iqn_loss_rejects(built, case):
    _, change, word = case
    d = good_desc()
    d.n = 5                                       # (a call that would launch, were it accepted)
    LK.assert_rejected(N.load().sgw_iqn_loss, d, change, word)


def test_sgw_iqn_loss_null_desc_and_no_rows(built):
    lib = N.load()
    assert lib.sgw_iqn_loss(None, None) == N.EINVAL and b"desc is NULL" in lib.sgw_last_error()
    d = good_desc()
    assert lib.sgw_iqn_loss(C.byref(d), None) == N.OK                            # n == 0: nothing is launched
    d.out_grad_expected = d.out_next_actions = d.out_row_terms = d.out_td_error = None     # all four are optional
    d.workspace, d.workspace_bytes = None, 0                                     # no rows need no workspace
    d.actions, d.action_type = 4097, N.PPO_ACT_U8                                # uint8 actions need no alignment
    d.valid, d.valid_type = 4104, N.POLICY_F64
    d.num_quantiles, d.num_actions, d.discount = 64, 256, 0.0
    assert lib.sgw_iqn_loss(C.byref(d), None) == N.OK
    d.num_quantiles, d.num_actions, d.discount = 1, 1, -1.5
    assert lib.sgw_iqn_loss(C.byref(d), None) == N.OK


# ------------------------------------------------------------------------------------------------------------- the torch path
@pytest.mark.parametrize("tag", sorted(SETS))
def test_iqn_loss_torch_reproduces_the_reference(tag):
    s = SETS[tag]
    qe, taus, ql, qt, actions, rewards, dones, valid, discount = tensors(s)
    qe.requires_grad_(True)
    ql.requires_grad_(True)
    L, td, a_star, quant = losses._iqn_loss_torch(qe, taus, ql, qt, actions, rewards, dones, valid, discount)
    assert L.dtype == torch.float64 and td.dtype == torch.float32 and quant.dtype == torch.float64
    L.backward()
    info = LC.restate(*LC.inputs_of(s))
    LC.same_bits(td.detach().numpy(), s["td_error"], "td_error", tag)
    LC.same_bits(a_star.numpy(), info["next_actions"], "next_actions", tag)
    LC.same_bits(quant.detach().numpy(), info["ql"], "the elementwise quantile loss", tag)
    assert ql.grad is None
    LC.same_bits(qe.grad.numpy(), s["grad_expected"], "dL/dq_expected", tag)         # the same ops as the reference: the same bits
    assert float(L.detach()) == float(s["loss"])


def test_iqn_loss_terms_on_cpu_tensors_and_out():
    s = SETS["4_12_64"]
    args = tensors(s)
    info = LC.restate(*LC.inputs_of(s))
    res = losses.iqn_loss_terms(*args, row_terms=True, td_error=True)
    assert isinstance(res, losses.IQNLoss) and res._workspace is None and "num_quantiles=12" in repr(res)
    assert res.loss.dtype == torch.float64 and res.loss.dim() == 0 and float(res.loss) == float(s["loss"])
    LC.same_bits(res.grad_expected.numpy(), s["grad_expected"], "grad_expected")
    LC.same_bits(res.next_actions.numpy(), info["next_actions"], "next_actions")
    LC.same_bits(res.td_error.numpy(), s["td_error"], "td_error")
    within(res.row_terms.numpy(), info["row_terms"], 144 * 2.0 ** -53 * np.abs(info["ql"]).sum(axis=(1, 2)) + 1e-300, "row terms", "4_12_64")
    # flat shapes, uint8 actions; out= is overwritten in place
    qe, taus, ql, qt, actions, rewards, dones, valid, discount = args
    again = losses.iqn_loss_terms(qe, taus.reshape(64, 12), ql, qt, actions.reshape(64).to(torch.uint8), rewards.reshape(64), dones.reshape(64),
                                  valid.reshape(64), discount, out=res, td_error=True)
    assert again is res
    LC.same_bits(res.grad_expected.numpy(), s["grad_expected"], "grad_expected through out=")
    # float32 valid (what sgw_sample writes): torch then stays in float32 throughout, inside the gradient's bound
    f32 = losses.iqn_loss_terms(qe, taus, ql, qt, actions, rewards, dones, valid.float(), discount)
    within(at_action(f32.grad_expected.numpy(), s["actions"]), info["grad_at_action"], LC.tolerances(info)["grad"], "dL/dq_expected, float32 valid", "4_12_64")
    plain = losses.iqn_loss_terms(*args)
    assert plain.row_terms is None and plain.td_error is None


def test_wrappers_refuse_what_does_not_fit():
    s = SETS["5_8_37"]
    qe, taus, ql, qt, actions, rewards, dones, valid, discount = tensors(s)
    good = dict(q_expected=qe, taus=taus, q_next_local=ql, q_next_target=qt, actions=actions, rewards=rewards, dones=dones, valid=valid, discount=discount)

    def call(fn=losses.iqn_loss_terms, **change):
        return fn(**{**good, **change})

    call()
    for name in ("q_expected", "q_next_local", "q_next_target", "taus", "rewards", "dones"):
        with pytest.raises(TypeError, match=name):
            call(**{name: good[name].double()})                                   # float64 quantile tensors are out of scope
    with pytest.raises(TypeError, match="actions"):
        call(actions=actions.int())
    with pytest.raises(TypeError, match="valid"):
        call(valid=valid.long())
    with pytest.raises(TypeError, match="q_next_target"):
        call(q_next_target=qt.numpy())
    with pytest.raises(TypeError, match="q_expected"):
        call(fn=losses.iqn_loss, q_expected=qe.numpy())
    with pytest.raises(ValueError, match=r"\[B, N, A\]"):
        call(q_expected=qe.reshape(37 * 8, 5))
    with pytest.raises(ValueError, match="q_next_local"):
        call(q_next_local=ql[:, :7].contiguous())                                 # different quantile counts are out of scope
    with pytest.raises(ValueError, match="taus"):
        call(taus=taus.reshape(37, 1, 8))
    with pytest.raises(ValueError, match="rewards"):
        call(rewards=rewards[:36])
    with pytest.raises(ValueError, match="actions"):
        call(actions=actions.reshape(1, 37))
    with pytest.raises(ValueError, match="contiguous"):
        call(q_next_target=qt.transpose(1, 2).contiguous().transpose(1, 2))       # strided [B, N, A] inputs are out of scope
    with pytest.raises(ValueError, match="quantiles"):
        call(q_expected=torch.zeros(2, 65, 3), q_next_local=torch.zeros(2, 65, 3), q_next_target=torch.zeros(2, 65, 3))
    with pytest.raises(ValueError, match="actions"):
        call(q_expected=torch.zeros(2, 3, 257))
    with pytest.raises(ValueError, match="discount"):
        call(discount=float("nan"))
    with pytest.raises(ValueError, match="discount"):
        call(discount=float("inf"))
    with pytest.raises(TypeError, match="out="):
        call(out=object())
    other = losses.iqn_loss_terms(*tensors(SETS["3_2_37"]))
    with pytest.raises(ValueError, match="out="):
        call(out=other)
    with pytest.raises(ValueError, match="out="):
        call(out=call(), row_terms=True)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="dones is on"):
            call(q_expected=qe.cuda(), taus=taus.cuda(), q_next_local=ql.cuda(), q_next_target=qt.cuda(), actions=actions.cuda(),
                 rewards=rewards.cuda(), valid=valid.cuda())


def test_iqn_loss_backpropagates_to_a_leaf_on_cpu():
    s = SETS["9_13_37"]
    qe, taus, ql, qt, actions, rewards, dones, valid, discount = tensors(s)
    leaf = qe.clone().requires_grad_(True)
    other = ql.clone().requires_grad_(True)
    L = losses.iqn_loss(leaf * 1.0, taus, other, qt, actions, rewards, dones, valid, discount)
    assert L.dtype == torch.float64 and L.dim() == 0 and float(L.detach()) == float(s["loss"])
    (L * 3.0).backward()
    assert other.grad is None                                                      # connected to q_expected only
    LC.same_bits(leaf.grad.numpy(), (torch.from_numpy(s["grad_expected"]) * 3.0).numpy(), "3 x dL/dq_expected at the leaf")
    with torch.no_grad():
        assert not losses.iqn_loss(qe, taus, ql, qt, actions, rewards, dones, valid, discount).requires_grad
