"""PPO's clipped loss without a GPU: the NumPy restatement of ``sgw_ppo_loss``'s semantics (``tests/ppo_loss_common.py``) against what the
reference's ``PyTorchPPO.train_step`` computed (``tests/golden/ppo_loss``) -- the mean loss, ``evaluate``'s log-probabilities and entropies
and the gradients at the actor's and the critic's outputs, each within its tolerance FORMULA --, the declaration of the entry points and
the layout of ``sgw_ppo_loss_desc`` against gcc, every descriptor the call rejects (validation precedes the launch, so no device is
needed), ``_ppo_loss_torch`` against the fixture, what the Python wrappers refuse, and ``ppo_loss`` on CPU tensors backpropagating to
leaf tensors."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from sorrel_amd import _native as N
from sorrel_amd import losses
from sorrel_amd.models import ActionLogits, ActionProbs
from tests import helpers as H
from tests import learner_common as LK
from tests import ppo_loss_common as LC

SETS, E2E = LC.load_fixture()


def within(got, want, tol, what, ctx):
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    share = float(np.max(err / np.maximum(tol, 1e-300))) if np.size(err) else 0.0
    print(f"{ctx} {what}: {share:.4f} of the tolerance")
    assert share <= 1.0, (ctx, what, share)


def restated(s, **kw):
    return LC.restate(s["probs"], False, s["values"], s["actions"], s["old_log_probs"], s["returns"], s["eps_clip"], s["entropy_coef"], **kw)


# ------------------------------------------------------------------------------------------------------------- restatement against the reference
@pytest.mark.parametrize("tag", sorted(SETS))
def test_restatement_reproduces_the_reference(tag):
    s = SETS[tag]
    info = restated(s)
    assert not info["bad"].any() and info["n"] == s["T"] and info["na"] == s["na"]
    mar = LC.branch_margins(info)
    assert mar["ratio"] > LC.MARGIN and mar["surrogates"] > LC.MARGIN                # equal branches are the fixture's condition
    assert s["exact"] or mar["clamp_rows"].min() > LC.MARGIN
    if s["T"] >= 37:
        assert all(v > 0 for v in LC.classes(info).values()), LC.classes(info)       # every gradient class occurs
    tol = LC.tolerances(info)
    within(info["lp"], s["log_probs"], tol["lp"], "log-probabilities", tag)
    within(info["H"], s["entropies"], tol["H"], "entropies", tag)
    within(info["grad_dist"], s["grad_probs"], tol["grad_dist"], "dL/dprobs", tag)
    within(info["grad_values"], s["grad_values"], tol["grad_values"], "dL/dvalues", tag)
    within(info["L"], s["loss"], tol["L"], "mean loss", tag)
    assert np.abs(s["grad_probs"]).max() > 1e-4 and np.abs(s["grad_values"]).max() > 1e-4      # (the bounds are not met by zeros)


def test_restatement_ties_invalid_rows_and_modes():
    rng = np.random.default_rng(5)
    n, na = 12, 5
    p = rng.integers(1, 9, size=(n, na)).astype(np.float64) / 64.0
    v, R = rng.normal(size=n), rng.normal(size=n)
    a = rng.integers(0, na, size=n)
    base = LC.restate(p, False, v, a, np.zeros(n, np.float32), R, 0.2, 0.01)
    old = base["lp"].astype(np.float32)
    # a tie: one action has q = 1, so lp = log(1 - 2^-52) = -2^-52, which a float32 holds: the ratio is exactly 1 and, with eps_clip 0,
    # s1 == s2 inside the (one-point) range -> the whole of A; with A == 0 a tie outside the range gives 0
    ones = np.full((4, 1), 3.0)
    A = np.array([1.0, -1.0, 2.0, 0.0])
    t = LC.restate(ones, False, np.zeros(4), np.zeros(4, np.int64), np.full(4, -2.0 ** -52, np.float32), A, 0.0, 0.0)
    assert (t["lp"] == -2.0 ** -52).all() and (t["r"] == 1.0).all() and (t["s1"] == t["s2"]).all() and t["inside"].all()
    assert np.array_equal(t["gr"], A) and np.array_equal(t["P"], -A)
    assert (t["grad_dist"] == 0.0).all()                                              # (q = 1 is clamped: nothing flows to the weights)
    t = LC.restate(ones, False, np.ones(4), np.zeros(4, np.int64), np.full(4, 0.5, np.float32), np.ones(4), 0.2, 0.0)
    assert (t["s1"] == t["s2"]).all() and not t["inside"].any() and (t["gr"] == 0.0).all()
    # logits = log of the weights give the same numbers within the tolerances; a power-of-two scale of the weights changes only S
    i1 = LC.restate(p, False, v, a, old, R, 0.2, 0.01)
    i2 = LC.restate(np.log(p), True, v, a, old, R, 0.2, 0.01)
    tol = LC.tolerances(i2)
    assert (np.abs(i1["lp"] - i2["lp"]) <= tol["lp"]).all() and abs(i1["L"] - i2["L"]) <= tol["L"]
    i3 = LC.restate(p * 8.0, False, v, a, old, R, 0.2, 0.01)
    assert np.array_equal(i1["lp"], i3["lp"]) and np.array_equal(i1["grad_dist"], i3["grad_dist"] * 8.0) and i1["L"] == i3["L"]
    # the gradient of the logits is the chain rule through softmax of the gradient of the probabilities
    q = i1["q"]
    gp = i1["grad_dist"] * i1["S"][:, None]                                           # dL/dq (S = sum of the weights)
    chain = q * (gp - (gp * q).sum(axis=1, keepdims=True))
    assert np.abs(chain - i2["grad_dist"]).max() <= 1e-12
    # invalid rows: NaN for the row and the means, neighbours untouched
    bad = p.copy()
    bad[2, 1] = -0.25
    bad[5, 0] = np.nan
    bad[7] = 0.0
    acts = a.copy()
    acts[9] = na
    acts[10] = -1
    ib = LC.restate(bad, False, v, acts, old, R, 0.2, 0.01)
    assert ib["bad"].nonzero()[0].tolist() == [2, 5, 7, 9, 10] and np.isnan(ib["L"]) and np.isnan(ib["Pm"])
    good = ~ib["bad"]
    assert np.isnan(ib["grad_dist"][~good]).all() and np.isnan(ib["grad_values"][~good]).all() and np.isnan(ib["P"][~good]).all()
    assert np.array_equal(ib["grad_dist"][good], i1["grad_dist"][good]) and np.array_equal(ib["H"][good], i1["H"][good])
    il = LC.restate(np.array([[0.0, np.inf, 1.0], [-np.inf, -np.inf, -np.inf], [np.nan, 0.0, 0.0], [-np.inf, 0.0, -np.inf]]), True,
                    np.zeros(4), np.array([0, 0, 0, 1]), np.zeros(4, np.float32), np.ones(4), 0.2, 0.01)
    assert il["bad"].tolist() == [True, True, True, False]


# ------------------------------------------------------------------------------------------------------------- header and binding
def test_header_declares_the_entry_points_and_the_binding_mirrors_them(built):
    text = open(os.path.join(H.ROOT, "include", "sgw.h")).read()
    assert re.search(r"int sgw_ppo_loss\(const sgw_ppo_loss_desc\* desc, void\* stream\);", text)
    assert re.search(r"int64_t sgw_ppo_loss_workspace_bytes\(int64_t n\);", text)
    lib = N.load()
    assert lib.sgw_version() == b"sgw 0.3 (gfx950)"                            # the additions are append-only
    blocks = LC.max_blocks()
    assert blocks >= 2
    assert lib.sgw_ppo_loss_workspace_bytes(0) == 0 and lib.sgw_ppo_loss_workspace_bytes(1) == 24 and lib.sgw_ppo_loss_workspace_bytes(257) == 48
    assert lib.sgw_ppo_loss_workspace_bytes(1 << 40) == blocks * 24
    assert lib.sgw_ppo_loss_workspace_bytes(-1) == N.EINVAL and b"n =" in lib.sgw_last_error()
    assert lib.sgw_ppo_loss_workspace_bytes((1 << 63) - 1) == N.EINVAL and lib.sgw_ppo_loss_workspace_bytes(1 << 58) == N.EINVAL      # (no overflow)


# ------------------------------------------------------------------------------------------------------------- refusals
def good_desc():
    """A descriptor the call accepts (the pointers are never followed: every test below is rejected, or has n == 0)."""
    d = N.SgwPpoLossDesc()
    d.dist = d.values = d.actions = d.old_log_probs = d.returns = 4096
    d.out_grad_dist = d.out_grad_values = d.out_row_terms = d.out_terms = d.workspace = 8192
    d.workspace_bytes = 1 << 20
    d.n, d.row_stride, d.num_actions = 0, 6, 5
    d.eps_clip, d.entropy_coef, d.value_coef = 0.2, 0.01, 0.5
    d.dist_type, d.mode, d.value_type, d.action_type, d.returns_type = N.POLICY_F32, N.POLICY_PROBS, N.POLICY_F32, N.PPO_ACT_I64, N.POLICY_F32
    return d


REJECTED = [
    ("dist is NULL", {"dist": None}, b"must not be NULL"),
    ("values is NULL", {"values": None}, b"must not be NULL"),
    ("actions is NULL", {"actions": None}, b"must not be NULL"),
    ("old_log_probs is NULL", {"old_log_probs": None}, b"must not be NULL"),
    ("returns is NULL", {"returns": None}, b"must not be NULL"),
    ("out_terms is NULL", {"out_terms": None}, b"must not be NULL"),
    ("n < 0", {"n": -1}, b"n ="),
    ("num_actions < 1", {"num_actions": 0}, b"num_actions"),
    ("num_actions > 256", {"num_actions": 257, "row_stride": 300}, b"num_actions"),
    ("row stride below num_actions", {"row_stride": 4}, b"row_stride"),
    ("unknown dist_type", {"dist_type": 2}, b"dist_type"),
    ("negative dist_type", {"dist_type": -1}, b"dist_type"),
    ("unknown mode", {"mode": 2}, b"mode"),
    ("unknown value_type", {"value_type": 2}, b"value_type"),
    ("unknown action_type", {"action_type": 2}, b"action_type"),
    ("negative action_type", {"action_type": -1}, b"action_type"),
    ("unknown returns_type", {"returns_type": 3}, b"returns_type"),
    ("reserved0 set", {"reserved0": 1}, b"reserved"),
    ("reserved1 set", {"reserved1": 1}, b"reserved"),
    ("negative eps_clip", {"eps_clip": -0.1}, b"eps_clip"),
    ("infinite eps_clip", {"eps_clip": float("inf")}, b"eps_clip"),
    ("NaN eps_clip", {"eps_clip": float("nan")}, b"eps_clip"),
    ("misaligned float32 dist", {"dist": 4098}, b"dist"),
    ("float64 dist on a 4-byte boundary", {"dist": 4100, "dist_type": N.POLICY_F64}, b"dist"),
    ("misaligned out_grad_dist", {"out_grad_dist": 8194}, b"out_grad_dist"),
    ("float64 values on a 4-byte boundary", {"values": 4100, "value_type": N.POLICY_F64}, b"values"),
    ("misaligned out_grad_values", {"out_grad_values": 8193}, b"out_grad_values"),
    ("float64 returns on a 4-byte boundary", {"returns": 4100, "returns_type": N.POLICY_F64}, b"returns"),
    ("misaligned old_log_probs", {"old_log_probs": 4098}, b"old_log_probs"),
    ("misaligned int64 actions", {"actions": 4100}, b"actions"),
    ("misaligned out_row_terms", {"out_row_terms": 8196}, b"float64"),
    ("misaligned out_terms", {"out_terms": 8196}, b"float64"),
    ("misaligned workspace", {"workspace": 8196}, b"float64"),
    ("no workspace", {"workspace": None}, b"workspace"),
    ("a workspace that is too small", {"workspace_bytes": 23}, b"workspace"),
    ("a workspace too small for two tiles", {"n": 257, "workspace_bytes": 47}, b"workspace"),
    ("offsets past 64 bits", {"n": 1 << 40, "row_stride": 1 << 30}, b"64-bit"),
]


@pytest.mark.parametrize("case", REJECTED, ids=[c[0] for c in REJECTED])
def test_sgw_ppo_loss_rejects(built, case):
    _, change, word = case
    d = good_desc()
    d.n = 5                                       # (a call that would launch, were it accepted)
    LK.assert_rejected(N.load().sgw_ppo_loss, d, change, word)


def test_sgw_ppo_loss_null_desc_and_no_rows(built):
    lib = N.load()
    assert lib.sgw_ppo_loss(None, None) == N.EINVAL and b"desc is NULL" in lib.sgw_last_error()
    d = good_desc()
    assert lib.sgw_ppo_loss(C.byref(d), None) == N.OK                            # n == 0: nothing is launched
    d.out_grad_dist = d.out_grad_values = d.out_row_terms = None                 # all three are optional
    d.workspace, d.workspace_bytes = None, 0                                     # no rows need no workspace
    d.actions, d.action_type = 4097, N.PPO_ACT_U8                                # uint8 actions need no alignment
    d.dist, d.mode = 4100, N.POLICY_LOGITS                                       # float32 rows need 4-byte alignment only
    d.num_actions, d.row_stride, d.eps_clip = 256, 256, 0.0
    assert lib.sgw_ppo_loss(C.byref(d), None) == N.OK


# ------------------------------------------------------------------------------------------------------------- the torch path
@pytest.mark.parametrize("tag", sorted(SETS))
def test_ppo_loss_torch_reproduces_the_reference(tag):
    s = SETS[tag]
    info = restated(s)
    tol = LC.tolerances(info)
    probs = torch.tensor(s["probs"], requires_grad=True)
    values = torch.tensor(s["values"], requires_grad=True)
    L, Pm, M, Hm, P, sq, Hrow = losses._ppo_loss_torch(probs, False, values, torch.tensor(s["actions"]), torch.tensor(s["old_log_probs"]),
                                                       torch.tensor(s["returns"]), s["eps_clip"], s["entropy_coef"])
    L.backward()
    within(L.item(), s["loss"], tol["L"], "mean loss", tag)
    within(Hrow.detach().numpy(), s["entropies"], tol["H"], "entropies", tag)
    within(P.detach().numpy(), info["P"], tol["P"], "policy terms", tag)
    within(probs.grad.numpy(), s["grad_probs"], tol["grad_dist"], "dL/dprobs", tag)
    within(values.grad.numpy(), s["grad_values"], tol["grad_values"], "dL/dvalues", tag)
    within([Pm.item(), M.item(), Hm.item()], [info["Pm"], info["M"], info["Hm"]], np.array([tol["Pm"], tol["M"], tol["Hm"]]), "means", tag)


def test_ppo_loss_terms_on_cpu_tensors_and_out():
    s = SETS[sorted(SETS)[2]]
    info = restated(s, value_coef=0.25)
    tol = LC.tolerances(info)
    args = (torch.tensor(s["values"]), torch.tensor(s["actions"]), torch.tensor(s["old_log_probs"]), torch.tensor(s["returns"]), s["eps_clip"], s["entropy_coef"])
    res = losses.ppo_loss_terms(ActionProbs(torch.tensor(s["probs"])), *args, 0.25, row_terms=True)
    assert isinstance(res, losses.PPOLoss) and res.loss.dim() == 0 and res.loss.dtype == torch.float64 and "PPOLoss" in repr(res)
    within(res.terms.numpy(), [info["L"], info["Pm"], info["M"], info["Hm"]], np.array([tol["L"], tol["Pm"], tol["M"], tol["Hm"]]), "terms", "cpu")
    within(res.grad_dist.numpy(), info["grad_dist"], tol["grad_dist"], "dL/dprobs", "cpu")
    within(res.grad_values.numpy(), info["grad_values"], tol["grad_values"], "dL/dvalues", "cpu")
    within(res.row_terms.numpy(), np.stack([info["P"], info["d2"], info["H"]], axis=1), np.stack([tol["P"], tol["d2"], tol["H"]], axis=1), "row terms", "cpu")
    # a bare tensor is probabilities; logits = log of them give the same loss; out= hands back the same object, overwritten
    again = losses.ppo_loss_terms(torch.tensor(s["probs"]), *args, 0.25, out=res)
    assert again is res
    lg = losses.ppo_loss_terms(ActionLogits(torch.tensor(np.log(s["probs"]))), *args, 0.25)
    il = LC.restate(np.log(s["probs"]), True, s["values"], s["actions"], s["old_log_probs"], s["returns"], s["eps_clip"], s["entropy_coef"], 0.25)
    within(lg.grad_dist.numpy(), il["grad_dist"], LC.tolerances(il)["grad_dist"], "dL/dlogits", "cpu")
    # leading shapes: a [count, E] segment with the distribution its [count * E, A] view; float32 inputs
    T = s["T"] // 2 * 2
    seg = losses.ppo_loss_terms(torch.tensor(s["probs"][:T]).float(), torch.tensor(s["values"][:T]).float().view(2, T // 2),
                                torch.tensor(s["actions"][:T]).to(torch.uint8).view(2, T // 2), torch.tensor(s["old_log_probs"][:T]).view(2, T // 2),
                                torch.tensor(s["returns"][:T]).float().view(2, T // 2), s["eps_clip"], s["entropy_coef"])
    assert seg.grad_values.shape == (2, T // 2) and seg.grad_values.dtype == torch.float32 and seg.grad_dist.dtype == torch.float32
    assert seg.row_terms is None and torch.isfinite(seg.loss)


def test_wrappers_refuse_what_does_not_fit():
    n, na = 6, 3
    p = torch.full((n, na), 1.0 / 3, dtype=torch.float64)
    v, a, old, R = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.int64), torch.zeros(n), torch.ones(n, dtype=torch.float64)
    ok = losses.ppo_loss_terms(p, v, a, old, R, 0.2, 0.01)
    for change, err in (
            (dict(values=torch.zeros(n + 1, dtype=torch.float64)), ValueError), (dict(actions=torch.zeros(n - 1, dtype=torch.int64)), ValueError),
            (dict(old=torch.zeros(2 * n)), ValueError), (dict(returns=torch.ones(1, dtype=torch.float64)), ValueError),
            (dict(values=torch.zeros(2 * n, dtype=torch.float64)[::2]), ValueError), (dict(old=torch.zeros(2 * n)[::2]), ValueError),
            (dict(returns=torch.ones((n, 2), dtype=torch.float64)[:, 0]), ValueError), (dict(actions=torch.zeros((n, 2), dtype=torch.int64)[:, 1]), ValueError),
            (dict(dist=torch.full((na, n), 0.5, dtype=torch.float64).t()), ValueError), (dict(dist=torch.zeros(n)), ValueError),
            (dict(dist=torch.zeros((n, 257))), ValueError),
            (dict(values=torch.zeros(n, dtype=torch.float16)), TypeError), (dict(actions=torch.zeros(n, dtype=torch.int32)), TypeError),
            (dict(old=torch.zeros(n, dtype=torch.float64)), TypeError), (dict(returns=torch.ones(n, dtype=torch.int64)), TypeError),
            (dict(dist=p.half()), TypeError), (dict(dist=p.numpy()), TypeError), (dict(values=[0.0] * n), TypeError),
            (dict(eps=-0.5), ValueError), (dict(eps=float("inf")), ValueError),
            (dict(out=object()), TypeError), (dict(out=losses.PPOLoss(p[:3], v[:3])), ValueError), (dict(out=ok, row_terms=True), ValueError)):
        kw = dict(dist=p, values=v, actions=a, old=old, returns=R, eps=0.2)
        extra = {k: change.pop(k) for k in ("out", "row_terms") if k in change}
        kw.update(change)
        with pytest.raises(err):
            losses.ppo_loss_terms(kw["dist"], kw["values"], kw["actions"], kw["old"], kw["returns"], kw["eps"], 0.01, **extra)
    with pytest.raises(ValueError):
        losses.ppo_loss(p, v[:3], a, old, R, 0.2, 0.01)
    with pytest.raises(TypeError):
        losses.ppo_loss(p, [0.0] * n, a, old, R, 0.2, 0.01)
    stale = losses.ppo_loss_terms(p, v, a, old, R, 0.2, 0.01, row_terms=True)
    stale.row_terms = stale.row_terms[:3]                                        # row terms of another row count
    with pytest.raises(ValueError):
        losses.ppo_loss_terms(p, v, a, old, R, 0.2, 0.01, out=stale, row_terms=True)
    # a wider row stride is a layout the call takes: the gradient has the same strides
    wide = torch.full((n, na + 2), 0.25, dtype=torch.float64)[:, :na]
    res = losses.ppo_loss_terms(wide, v, a, old, R, 0.2, 0.01)
    assert res.grad_dist.stride() == wide.stride() and torch.allclose(res.grad_dist * 0.75, ok.grad_dist, rtol=1e-12, atol=1e-18)


def test_ppo_loss_backpropagates_to_leaves_on_cpu():
    s = SETS[sorted(SETS)[3]]
    info = restated(s)
    tol = LC.tolerances(info)
    probs = torch.tensor(s["probs"], requires_grad=True)
    values = torch.tensor(s["values"], requires_grad=True)
    L = losses.ppo_loss(ActionProbs(probs), values, torch.tensor(s["actions"]), torch.tensor(s["old_log_probs"]), torch.tensor(s["returns"]),
                        s["eps_clip"], s["entropy_coef"])
    assert L.dim() == 0 and L.dtype == torch.float64 and L.requires_grad
    within(L.item(), s["loss"], tol["L"], "mean loss", "autograd")
    (3.0 * L).backward()                                                         # the incoming gradient multiplies the saved ones
    within(probs.grad.numpy() / 3.0, s["grad_probs"], tol["grad_dist"] + 4 * LC.U * np.abs(s["grad_probs"]), "dL/dprobs", "autograd")
    within(values.grad.numpy() / 3.0, s["grad_values"], tol["grad_values"] + 4 * LC.U * np.abs(s["grad_values"]), "dL/dvalues", "autograd")
    # through a network's last layer: the parameters of a softmax head receive a gradient
    head = torch.nn.Linear(4, s["na"]).double()
    x = torch.tensor(np.linspace(-1, 1, s["T"] * 4).reshape(s["T"], 4))
    L = losses.ppo_loss(ActionLogits(head(x)), values.detach(), torch.tensor(s["actions"]), torch.tensor(s["old_log_probs"]), torch.tensor(s["returns"]),
                        s["eps_clip"], s["entropy_coef"])
    L.backward()
    assert head.weight.grad is not None and head.weight.grad.abs().max() > 0 and torch.isfinite(head.weight.grad).all()
