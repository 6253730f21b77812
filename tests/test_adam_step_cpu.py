"""``sgw_adam_step`` without a GPU: the NumPy restatement of its contract (``tests/adam_step_common.py``) against what the reference's own
``iRainbowModel.train_step`` and ``PyTorchPPO.train_step`` did to their parameters (``tests/golden/adam_step``) -- Adam's moments and the
targets bit for bit, the parameters and the norm each within its tolerance FORMULA --, ``_adam_step_torch`` through ``FusedAdam`` on CPU
tensors against the same fixture, the layouts of the four structs against gcc, every refusal of ``sgw_adam_plan`` / ``sgw_adam_step``
(validation precedes the launch, so no device is needed), the chunk map, the order of the norm's merge, a ``state_dict`` round trip
with ``torch.optim.Adam`` both ways and the agreement between the header and ``EXPORTS``."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from sorrel_amd import _native as N
from sorrel_amd import optim
from tests import adam_step_common as AC
from tests import helpers as H
from tests import learner_common as LK

FIX = {name: AC.load_fixture(name) for name in ("iqn", "ppo")}


def share(got, want, tol, what, ctx):
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    part = float(np.max(err / np.maximum(tol, 1e-300))) if np.size(err) else 0.0
    print(f"{ctx} {what}: {part:.4f} of the tolerance")
    assert part <= 1.0, (ctx, what, part)


def hyper(meta):
    return dict(beta1=meta["betas"][0], beta2=meta["betas"][1], eps=meta["eps"], tau=meta["tau"] or 0.0)


# ------------------------------------------------------------------------------------------------------------- restatement against the reference
def test_the_fixture_covers_what_the_issue_lists():
    iqn, ppo = FIX["iqn"], FIX["ppo"]
    assert iqn["meta"]["tensors"] == 16 and iqn["meta"]["steps"] == 4 and iqn["meta"]["dtype"] == "float32"
    assert 1 in [int(np.prod(s)) for s in iqn["meta"]["shapes"]]
    norms = [float(s["norm"]) for s in iqn["steps"]]
    assert any(n > 1 for n in norms) and any(n < 1 for n in norms)
    assert ppo["meta"]["dtype"] == "float64" and ppo["meta"]["steps"] == 3 and len(set(ppo["meta"]["lrs"])) == 2
    for f in FIX.values():
        assert os.path.getsize(f["path"]) < 200 * 1024
        assert max(f["meta"]["share"].values()) <= 0.5 and f["meta"]["moments_exact"]
        for s in f["steps"]:
            assert all(a.dtype == np.dtype(f["meta"]["dtype"]) for a in s["grad"] + s["param_after"])


@pytest.mark.parametrize("name", sorted(FIX))
def test_restatement_reproduces_the_reference(name):
    meta, steps = FIX[name]["meta"], FIX[name]["steps"]
    dtype, clipped = np.dtype(meta["dtype"]), meta["max_norm"] is not None
    for s, rec in enumerate(steps):
        ctx = f"{name} step {s}"
        coef = AC.torch_clip_coef(rec["norm"], meta["max_norm"], dtype) if clipped else None
        got = AC.restate(AC.fixture_tensors(rec, meta["lrs"], clipped), dtype, clip_mode=AC.CLIP_COEF if clipped else AC.CLIP_NONE, coef=coef,
                         step=s + 1, **hyper(meta))
        for k, t in enumerate(got["tensors"]):
            AC.same_bits(t["m"], rec["exp_avg_after"][k], f"exp_avg {k}", ctx)
            AC.same_bits(t["v"], rec["exp_avg_sq_after"][k], f"exp_avg_sq {k}", ctx)
            if clipped:
                AC.same_bits(t["t"], rec["target_after"][k], f"target {k}", ctx)
            share(t["p"], rec["param_after"][k], AC.param_tolerance(rec["param_after"][k], rec["param_before"][k], dtype), f"param {k}", ctx)
            assert not np.array_equal(rec["param_after"][k], rec["param_before"][k])           # (the bound is not met by standing still)
        if clipped:
            mine = AC.restate(AC.fixture_tensors(rec, meta["lrs"], True), dtype, clip_mode=AC.CLIP_NORM, max_norm=meta["max_norm"], step=s + 1,
                              **hyper(meta))
            n_total = sum(g.size for g in rec["grad"])
            share(mine["norm"], float(rec["norm"]), AC.norm_tolerance(n_total, mine["norm"], dtype), "norm", ctx)
            assert (mine["c"] < 1) == (float(rec["norm"]) > 1)


def test_restatement_device_state_against_by_value():
    """Running products against pow: the same tensors stepped three times both ways stay inside ``device_step_tolerance``."""
    meta, rec = FIX["ppo"]["meta"], FIX["ppo"]["steps"][0]
    dtype = np.dtype(meta["dtype"])
    a = b = AC.fixture_tensors(rec, meta["lrs"], False)
    state = AC.fresh_state()
    for t in range(1, 4):
        before = [x["p"] for x in a]
        ra = AC.restate(a, dtype, step=t, **hyper(meta))
        rb = AC.restate(b, dtype, state=state, **hyper(meta))
        state = rb["state"]
        assert state[0] == t
        for k, (x, y) in enumerate(zip(ra["tensors"], rb["tensors"])):
            share(y["p"], x["p"], AC.device_step_tolerance(x["p"], before[k], t, dtype), f"param {k}", f"t = {t}")
        a, b = ra["tensors"], rb["tensors"]


# ------------------------------------------------------------------------------------------------------------- the torch path
def fused_on_cpu(name, s):
    meta, rec = FIX[name]["meta"], FIX[name]["steps"][s]
    clipped = meta["max_norm"] is not None
    params = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in rec["param_before"]]
    targets = [torch.from_numpy(a.copy()) for a in rec["target_before"]] if clipped else None
    lrs = meta["lrs"]
    groups = [dict(params=[p for p, lr in zip(params, lrs) if lr == value], lr=value) for value in dict.fromkeys(lrs)]
    opt = optim.FusedAdam(groups, betas=tuple(meta["betas"]), eps=meta["eps"], max_grad_norm=meta["max_norm"], target_params=targets, tau=meta["tau"])
    for k, p in enumerate(params):
        p.grad = torch.from_numpy(rec["grad"][k].copy())
        if s:
            opt.state[p] = dict(step=torch.tensor(float(s)), exp_avg=torch.from_numpy(rec["exp_avg_before"][k].copy()),
                                exp_avg_sq=torch.from_numpy(rec["exp_avg_sq_before"][k].copy()))
    return opt, params, targets, rec, meta


@pytest.mark.parametrize("name,s", [("iqn", 0), ("iqn", 1), ("iqn", 3), ("ppo", 0), ("ppo", 2)])
def test_adam_step_torch_reproduces_the_reference(name, s):
    opt, params, targets, rec, meta = fused_on_cpu(name, s)
    dtype = np.dtype(meta["dtype"])
    norm = opt.step()
    for k, p in enumerate(params):
        ctx = f"{name} step {s}"
        AC.same_bits(opt.state[p]["exp_avg"].numpy(), rec["exp_avg_after"][k], f"exp_avg {k}", ctx)
        AC.same_bits(opt.state[p]["exp_avg_sq"].numpy(), rec["exp_avg_sq_after"][k], f"exp_avg_sq {k}", ctx)
        share(p.detach().numpy(), rec["param_after"][k], AC.param_tolerance(rec["param_after"][k], rec["param_before"][k], dtype), f"param {k}", ctx)
        assert int(opt.state[p]["step"]) == s + 1
        if targets:
            AC.same_bits(targets[k].numpy(), rec["target_after"][k], f"target {k}", ctx)
            AC.same_bits(p.grad.numpy(), rec["grad_clipped"][k], f"clipped grad {k}", ctx)      # (the torch path IS the reference's lines)
    if targets:
        assert norm.dtype == torch.float64 and norm.dim() == 0
        n_total = sum(g.size for g in rec["grad"])
        share(float(norm), float(rec["norm"]), AC.norm_tolerance(n_total, float(rec["norm"]), dtype), "norm", f"{name} step {s}")
    else:
        assert norm is None


def test_fused_adam_refuses_and_skips_on_cpu():
    w = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError, match="beta1"):
        optim.FusedAdam([w], betas=(0.4, 0.999))
    with pytest.raises(ValueError, match="betas"):
        optim.FusedAdam([w], betas=(0.9, 1.0))
    with pytest.raises(ValueError, match="go together"):
        optim.FusedAdam([w], tau=0.1)
    with pytest.raises(ValueError, match="target_params"):
        optim.FusedAdam([w], target_params=[], tau=0.1)
    with pytest.raises(ValueError, match="target"):
        optim.FusedAdam([w], target_params=[torch.zeros(4)], tau=0.1)
    with pytest.raises(TypeError, match="float32 and float64"):
        optim.FusedAdam([torch.nn.Parameter(torch.zeros(3, dtype=torch.float16))])
    with pytest.raises(ValueError, match="max_grad_norm"):
        optim.FusedAdam([w], max_grad_norm=float("inf"))
    opt = optim.FusedAdam([w], zero_grads=True)
    assert opt.step() is None and len(opt.state) == 0                          # no gradient anywhere: nothing happens
    with pytest.raises(ValueError, match="closure"):
        opt.step(lambda: 0.0)
    w.grad = torch.ones(3)
    opt.step()
    assert not w.grad.any() and (w.detach() < 0).all()
    opt.zero_grad()
    assert w.grad is not None                                                  # set_to_none defaults to False here
    opt.zero_grad(set_to_none=True)
    assert w.grad is None


def test_state_dict_round_trips_with_torch_adam_both_ways():
    torch.manual_seed(0)
    a = [torch.nn.Parameter(torch.randn(5, 3, dtype=torch.float64)), torch.nn.Parameter(torch.randn(7, dtype=torch.float64))]
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    ours = optim.FusedAdam([dict(params=a[:1], lr=3e-4), dict(params=a[1:], lr=1e-3)])
    theirs = torch.optim.Adam([dict(params=b[:1], lr=3e-4), dict(params=b[1:], lr=1e-3)])
    assert set(ours.state_dict()["param_groups"][0]) == set(theirs.state_dict()["param_groups"][0])
    for _ in range(2):
        for p, q in zip(a, b):
            p.grad = torch.randn_like(p)
            q.grad = p.grad.clone()
        ours.step()
        theirs.step()
    sd_ours, sd_theirs = ours.state_dict(), theirs.state_dict()
    assert sd_ours["param_groups"] == sd_theirs["param_groups"]
    for k in sd_theirs["state"]:
        assert set(sd_ours["state"][k]) == set(sd_theirs["state"][k]) == {"step", "exp_avg", "exp_avg_sq"}
        assert float(sd_ours["state"][k]["step"]) == float(sd_theirs["state"][k]["step"]) == 2.0
        assert torch.equal(sd_ours["state"][k]["exp_avg"], sd_theirs["state"][k]["exp_avg"])
    # ours -> torch's and torch's -> ours, then one more step each: the same parameters
    ours2 = optim.FusedAdam([dict(params=a[:1], lr=1.0), dict(params=a[1:], lr=1.0)])
    theirs2 = torch.optim.Adam([dict(params=b[:1]), dict(params=b[1:])])
    ours2.load_state_dict(sd_theirs)
    theirs2.load_state_dict(sd_ours)
    assert [g["lr"] for g in ours2.param_groups] == [3e-4, 1e-3]
    for p, q in zip(a, b):
        p.grad = torch.randn_like(p)
        q.grad = p.grad.clone()
    ours2.step()
    theirs2.step()
    for p, q in zip(a, b):
        assert torch.equal(p.detach(), q.detach())
        assert float(ours2.state[p]["step"]) == float(theirs2.state[q]["step"]) == 3.0


# ------------------------------------------------------------------------------------------------------------- header and binding
def test_header_declares_the_entry_points_and_the_binding_mirrors_them(built):
    text = open(os.path.join(H.ROOT, "include", "sgw.h")).read()
    assert re.search(r"int64_t sgw_adam_plan_bytes\(int64_t num_tensors, int64_t total_numel\);", text)
    assert re.search(r"int sgw_adam_plan\(const sgw_adam_tensor\* records, int64_t num_tensors, int32_t dtype, void\* host_image, int64_t image_bytes, "
                     r"sgw_adam_plan_info\* info\);", text)
    assert re.search(r"int sgw_adam_step\(const sgw_adam_step_desc\* desc, void\* stream\);", text)
    assert (AC.CLIP_NONE, AC.CLIP_NORM, AC.CLIP_COEF) == (N.ADAM_CLIP_NONE, N.ADAM_CLIP_NORM, N.ADAM_CLIP_COEF)
    assert N.ADAM_MAX_TENSORS == AC.MAX_TENSORS and N.ADAM_CHUNK == AC.CHUNK
    lib = N.load()
    assert lib.sgw_version() == b"sgw 0.3 (gfx950)"                            # the additions are append-only
    pb = lib.sgw_adam_plan_bytes
    assert pb(1, 0) == 64 + 8 and pb(16, 808) == 16 * 72 and pb(1, 8193) == 64 + 3 * 8 and pb(4096, 1 << 40) == 4096 * 72 + (1 << 28) * 8
    assert pb(0, 5) == N.EINVAL and pb(4097, 5) == N.EINVAL and b"num_tensors" in lib.sgw_last_error()
    assert pb(3, -1) == N.EINVAL and b"total_numel" in lib.sgw_last_error()
    parts = open(os.path.join(H.ROOT, "__graft_entry__.py")).read()
    assert '"adam_step.h"' in parts and '#include "adam_step.h"' in open(os.path.join(H.ROOT, "sorrel_amd", "csrc", "sgw.hip")).read()


# ------------------------------------------------------------------------------------------------------------- the plan
def records(numels, base=1 << 20, grads=None, targets=True, step=1 << 16):
    """Records over made-up addresses (never followed: planning reads no tensor)."""
    recs = (N.SgwAdamTensor * len(numels))()
    for k, (r, n) in enumerate(zip(recs, numels)):
        at = base + 8 * k * step
        r.param, r.grad, r.exp_avg, r.exp_avg_sq, r.target = at, at + step, at + 2 * step, at + 3 * step, (at + 4 * step) if targets else None
        if grads is not None and not grads[k]:
            r.grad = None
        r.numel, r.lr = n, 1e-3 * (k + 1)
    return recs


def plan(recs, dtype=N.POLICY_F32, image_bytes=None):
    lib = N.load()
    size = lib.sgw_adam_plan_bytes(len(recs), sum(max(r.numel, 0) for r in recs))
    image = np.zeros((size if image_bytes is None else image_bytes) // 8 + 1, np.int64)
    info = N.SgwAdamPlanInfo()
    rc = lib.sgw_adam_plan(recs, len(recs), dtype, image.ctypes.data, size if image_bytes is None else image_bytes, C.byref(info))
    return rc, image, info


def test_the_chunk_map(built):
    numels = [0, 1, 4095, 4096, 4097, 8193, 5]
    grads = [True, True, True, True, True, True, False]
    recs = records(numels, grads=grads)
    recs[2].param += 4                                   # one base off 16 bytes: this tensor goes element by element
    rc, image, info = plan(recs)
    assert rc == N.OK
    want, first = AC.chunk_map(numels, grads)
    assert [AC.chunks_of(n) for n in numels] == [0, 1, 1, 1, 2, 3, 1]
    assert info.num_chunks == len(want) == 8 and info.workspace_bytes == 8 * 8 and info.total_numel == sum(numels[:6])
    T = len(numels)
    assert info.image_bytes == T * 64 + 8 * 8 <= N.load().sgw_adam_plan_bytes(T, sum(numels))
    raw = image.view(np.uint8)[:info.image_bytes]
    dev = np.frombuffer(raw[:T * 64].tobytes(), dtype=np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("t", "<u8"), ("numel", "<i8"),
                                                                 ("lr", "<f8"), ("first", "<i4"), ("flags", "<i4")]))
    assert dev["numel"].tolist() == numels and dev["first"].tolist() == first and dev["flags"].tolist() == [1, 1, 0, 1, 1, 1, 1]
    assert dev["p"].tolist() == [r.param for r in recs] and dev["g"].tolist() == [r.grad or 0 for r in recs]
    assert dev["lr"].tolist() == [r.lr for r in recs]
    cmap = np.frombuffer(raw[T * 64:].tobytes(), dtype="<i4").reshape(-1, 2)
    assert [tuple(x) for x in cmap.tolist()] == want
    rc, _, info = plan(records([3, 3], grads=[False, False]))
    assert rc == N.OK and info.num_chunks == 0 and info.workspace_bytes == 0 and info.image_bytes == 128


def test_the_merge_order():
    rng = np.random.default_rng(5)
    g = rng.normal(size=4096 + 37).astype(np.float32)
    # a chunk: lane t's sixteen elements serially, then the tree, written out
    x = g[:4096].astype(np.float64) ** 2
    lanes = []
    for t in range(256):
        acc = 0.0
        for r in range(4):
            for e in range(4):
                acc += x[4 * (t + 256 * r) + e]
        lanes.append(acc)

    def halve(v):
        return v[0] if len(v) == 1 else halve([v[i] + v[i + len(v) // 2] for i in range(len(v) // 2)])

    assert AC.chunk_sum(g[:4096]) == halve(lanes)
    tail = [float(v) ** 2 for v in g[4096:].astype(np.float64)]
    tail_lanes = [sum(tail[4 * t:4 * t + 4], 0.0) for t in range(256)]         # (37 elements: lanes 0..9, one group each)
    assert AC.chunk_sum(g[4096:]) == halve(tail_lanes)
    assert AC.tensor_sum(g) == AC.chunk_sum(g[:4096]) + AC.chunk_sum(g[4096:]) and AC.tensor_sum(None) == 0.0 and AC.tensor_sum(g[:0]) == 0.0
    S = rng.random(300)
    by_lane = [(S[i] + S[i + 256]) if i + 256 < 300 else S[i] for i in range(256)]
    assert AC.merge(S) == halve(by_lane) and AC.merge(S) != 0.0
    assert AC.grad_norm([g, None, g[:3]]) == float(np.sqrt(halve([AC.tensor_sum(g), 0.0, AC.tensor_sum(g[:3])] + [0.0] * 253)))
    # the coefficient: clipped above max_norm, 1 below it, NaN stays NaN
    assert AC.clip_coef(4.0, 1.0, np.float32) == np.float32(1.0) / (np.float32(4.0) + np.float32(1e-6))
    assert AC.clip_coef(0.25, 1.0, np.float32) == 1 and AC.clip_coef(0.0, 1.0, np.float64) == 1 and np.isnan(AC.clip_coef(float("nan"), 1.0, np.float32))
    assert AC.clip_coef(float("inf"), 1.0, np.float32) == 0


# ------------------------------------------------------------------------------------------------------------- refusals
PLAN_REJECTED = [
    ("param is NULL", dict(param=None), b"param must not be NULL"),
    ("exp_avg is NULL", dict(exp_avg=None), b"exp_avg"),
    ("exp_avg_sq is NULL", dict(exp_avg_sq=None), b"exp_avg_sq"),
    ("numel < 0", dict(numel=-1), b"numel"),
    ("infinite lr", dict(lr=float("inf")), b"lr"),
    ("NaN lr", dict(lr=float("nan")), b"lr"),
    ("reserved set", dict(reserved=1), b"reserved"),
] + [(f"misaligned {name}", {name: (1 << 20) + 2}, b"aligned") for name in ("param", "grad", "exp_avg", "exp_avg_sq", "target")]


@pytest.mark.parametrize("case", PLAN_REJECTED, ids=[c[0] for c in PLAN_REJECTED])
def test_sgw_adam_plan_rejects_a_record(built, case):
    _, change, word = case
    recs = records([5, 7, 9])
    for key, value in change.items():
        setattr(recs[1], key, value)
    rc, _, _ = plan(recs)
    assert rc == N.EINVAL
    msg = N.load().sgw_last_error()
    assert word in msg and b"tensor 1" in msg, msg


def test_sgw_adam_plan_rejects_a_call(built):
    lib = N.load()
    recs, info, image = records([5, 4097]), N.SgwAdamPlanInfo(), np.zeros(64, np.int64)
    good = lambda: [recs, 2, N.POLICY_F32, image.ctypes.data, image.nbytes, C.byref(info)]      # noqa: E731
    assert lib.sgw_adam_plan(*good()) == N.OK and info.num_chunks == 3
    for at, value, word in ((0, None, b"must not be NULL"), (3, None, b"must not be NULL"), (5, None, b"must not be NULL"), (1, 0, b"num_tensors"),
                            (1, 4097, b"num_tensors"), (2, 2, b"dtype"), (2, -1, b"dtype"), (3, image.ctypes.data + 4, b"8-byte"),
                            (4, 2 * 64 + 3 * 8 - 1, b"image needs"), (4, 0, b"image needs")):
        args = good()
        args[at] = value
        assert lib.sgw_adam_plan(*args) == N.EINVAL and word in lib.sgw_last_error(), (at, value, lib.sgw_last_error())
    recs64 = records([5, 7])
    recs64[0].grad += 4
    assert plan(recs64, N.POLICY_F32)[0] == N.OK and plan(recs64, N.POLICY_F64)[0] == N.EINVAL            # float64 on a 4-byte boundary
    skipped = records([5, 7], grads=[False, True])
    skipped[0].exp_avg = skipped[0].exp_avg_sq = None                                                       # a skipped tensor needs no state
    assert plan(skipped)[0] == N.OK
    huge = records([1 << 44])
    assert plan(huge, image_bytes=1 << 20)[0] == N.EINVAL and b"2^31" in lib.sgw_last_error()


def good_desc():
    """A descriptor the call accepts (no pointer is followed: every test below is rejected)."""
    d = N.SgwAdamStepDesc()
    d.plan, d.plan_bytes = 4096, 16 * 64 + 16 * 8
    d.clip_coef, d.out_norm, d.workspace, d.workspace_bytes = 8192, 8200, 16384, 16 * 8
    d.num_tensors, d.num_chunks, d.step = 16, 16, 1
    d.max_norm, d.beta1, d.beta2, d.eps, d.tau = 1.0, 0.9, 0.999, 1e-8, 0.01
    d.dtype, d.clip_mode, d.flags = N.POLICY_F32, N.ADAM_CLIP_NORM, N.ADAM_ZERO_GRADS
    return d


STEP_REJECTED = [
    ("plan is NULL", dict(plan=None), b"plan must not be NULL"),
    ("no tensors", dict(num_tensors=0), b"num_tensors"),
    ("too many tensors", dict(num_tensors=4097), b"num_tensors"),
    ("negative chunks", dict(num_chunks=-1), b"num_chunks"),
    ("2^31 chunks", dict(num_chunks=1 << 31), b"num_chunks"),
    ("unknown dtype", dict(dtype=2), b"dtype"),
    ("negative dtype", dict(dtype=-1), b"dtype"),
    ("unknown clip_mode", dict(clip_mode=3), b"clip_mode"),
    ("negative clip_mode", dict(clip_mode=-1), b"clip_mode"),
    ("unknown flag", dict(flags=2), b"flags"),
    ("reserved0 set", dict(reserved0=1), b"reserved"),
    ("reserved1 set", dict(reserved1=1), b"reserved"),
    ("beta1 = 1", dict(beta1=1.0), b"outside [0, 1)"),
    ("beta1 < 0", dict(beta1=-0.1), b"outside [0, 1)"),
    ("beta2 = 1", dict(beta2=1.0), b"outside [0, 1)"),
    ("beta2 < 0", dict(beta2=-0.5), b"outside [0, 1)"),
    ("1 - beta1 = 0.5", dict(beta1=0.5), b"below 0.5"),
    ("1 - beta1 above 0.5", dict(beta1=0.25), b"below 0.5"),
    ("step 0 without a state", dict(step=0), b"step ="),
    ("negative step", dict(step=-3), b"step ="),
    ("a step beside a state", dict(step_state=8192, step=2), b"step ="),
    ("COEF without a coefficient", dict(clip_mode=N.ADAM_CLIP_COEF, clip_coef=None), b"clip_coef"),
    ("misaligned clip_coef", dict(clip_coef=8194), b"clip_coef"),
    ("float64 clip_coef on a 4-byte boundary", dict(clip_coef=8196, dtype=N.POLICY_F64), b"clip_coef"),
    ("misaligned plan", dict(plan=4100), b"8-byte"),
    ("misaligned step_state", dict(step_state=8196, step=0), b"8-byte"),
    ("misaligned out_norm", dict(out_norm=8196), b"8-byte"),
    ("misaligned workspace", dict(workspace=16388), b"8-byte"),
    ("a short plan", dict(plan_bytes=16 * 64 + 16 * 8 - 1), b"plan of"),
    ("no workspace", dict(workspace=None), b"workspace"),
    ("a short workspace", dict(workspace_bytes=16 * 8 - 1), b"workspace"),
] + [(f"{how} {name}", {name: value}, b"finite") for name in ("max_norm", "beta1", "beta2", "eps", "tau")
     for how, value in (("infinite", float("inf")), ("NaN", float("nan")))]


@pytest.mark.parametrize("case", STEP_REJECTED, ids=[c[0] for c in STEP_REJECTED])
def test_sgw_adam_step_rejects(built, case):
    _, change, word = case
    d = good_desc()
    LK.assert_rejected(N.load().sgw_adam_step, d, change, word)


def test_sgw_adam_step_null_desc_and_nothing_to_do(built):
    lib = N.load()
    assert lib.sgw_adam_step(None, None) == N.EINVAL and b"desc is NULL" in lib.sgw_last_error()
    d = good_desc()
    d.num_chunks, d.plan_bytes, d.out_norm = 0, 16 * 64, None                   # every tensor skipped or empty, no norm asked for: no launch
    d.workspace, d.workspace_bytes = None, 0
    assert lib.sgw_adam_step(C.byref(d), None) == N.OK
    d.clip_mode, d.clip_coef = N.ADAM_CLIP_NONE, None
    assert lib.sgw_adam_step(C.byref(d), None) == N.OK
