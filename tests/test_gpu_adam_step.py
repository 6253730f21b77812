"""``sgw_adam_step`` on the device.  Every kernel output is compared bit for bit with the NumPy restatement of the contract
(``tests/adam_step_common.py``); against the reference's recorded steps (``tests/golden/adam_step``) the moments and targets are compared
bit for bit, the parameters and the norm by the formulas there.  All buffers of a call -- tensors, plan, workspace, scalars -- lie in one
arena with guard bytes between them, which must come back untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

from sorrel_amd import _native as N
from sorrel_amd import optim
from tests import adam_step_common as AC

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xA5
FIX = {name: AC.load_fixture(name) for name in ("iqn", "ppo")}
NUMELS = (1, 3, 4, 5, 1023, 1025, 4095, 4096, 4097, 8193)


class Arena:
    """Regions of one device buffer, each 64-byte aligned plus ``off`` bytes, ``GUARD`` filler bytes around every one."""

    def __init__(self):
        self.items, self.size = [], GUARD

    def add(self, nbytes, off=0):
        start = (self.size + 63) // 64 * 64 + off
        self.items.append((start, nbytes))
        self.size = start + nbytes + GUARD
        return len(self.items) - 1

    def finish(self):
        self.host = np.full(self.size + 64, FILL, np.uint8)
        self.dev = torch.empty(self.size + 64, dtype=torch.uint8, device="cuda")
        self.base = self.dev.data_ptr()
        assert self.base % 64 == 0

    def put(self, h, arr):
        start, n = self.items[h]
        raw = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        assert raw.size == n
        self.host[start:start + n] = raw

    def ptr(self, h):
        return self.base + self.items[h][0]

    def upload(self):
        self.dev.copy_(torch.from_numpy(self.host))

    def download(self):
        torch.cuda.synchronize()
        self.out = self.dev.cpu().numpy()
        guard = np.ones(self.out.size, bool)
        for start, n in self.items:
            guard[start:start + n] = False
        assert (self.out[guard] == FILL).all(), "a guard byte was written"

    def get(self, h, dtype, shape):
        start, n = self.items[h]
        return self.out[start:start + n].copy().view(dtype).reshape(shape)


def make(numels, dtype, seed, skip=(), no_target=(), scale=1.0):
    rng = np.random.default_rng(seed)
    out = []
    for k, n in enumerate(numels):
        g = None if k in skip else (rng.normal(size=n) * scale).astype(dtype)
        out.append(dict(p=rng.normal(size=n).astype(dtype), g=g, m=(rng.normal(size=n) * 0.1).astype(dtype),
                        v=(rng.random(size=n) * 0.01).astype(dtype), t=None if k in no_target else rng.normal(size=n).astype(dtype),
                        lr=1e-3 * (1 + k % 3)))
    return out


def run_abi(tensors, dtype, *, clip_mode=AC.CLIP_NONE, max_norm=1.0, coef=None, beta1=0.9, beta2=0.999, eps=1e-8, tau=0.0, step=None,
            state=None, zero_grads=False, misalign=False, calls=1):
    """One plan and ``calls`` steps through the C ABI on guarded buffers.  Returns dict(tensors, norm, c, state) as ``AC.restate`` does."""
    dtype = np.dtype(dtype)
    lib, ar = N.load(), Arena()
    off = dtype.itemsize if misalign else 0
    handles = []
    for t in tensors:
        handles.append({k: ar.add(t[k].nbytes, off) for k in ("p", "g", "m", "v", "t") if t[k] is not None})
    cmap, _ = AC.chunk_map([t["p"].size for t in tensors], [t["g"] is not None for t in tensors])
    T = len(tensors)
    image_bytes = T * 64 + len(cmap) * 8
    h_plan, h_ws, h_norm = ar.add(image_bytes), ar.add(len(cmap) * 8), ar.add(16)
    h_coef, h_state = ar.add(dtype.itemsize), ar.add(24)
    ar.finish()
    recs = (N.SgwAdamTensor * T)()
    for r, t, h in zip(recs, tensors, handles):
        r.param, r.exp_avg, r.exp_avg_sq = ar.ptr(h["p"]), ar.ptr(h["m"]), ar.ptr(h["v"])
        r.grad = ar.ptr(h["g"]) if "g" in h else None
        r.target = ar.ptr(h["t"]) if "t" in h else None
        r.numel, r.lr = t["p"].size, t["lr"]
        for k, hk in h.items():
            ar.put(hk, t[k])
    image = np.zeros(lib.sgw_adam_plan_bytes(T, sum(t["p"].size for t in tensors)) // 8 + 1, np.int64)
    info = N.SgwAdamPlanInfo()
    N.check(lib.sgw_adam_plan(recs, T, N.POLICY_F64 if dtype == np.float64 else N.POLICY_F32, image.ctypes.data, image.nbytes, C.byref(info)))
    assert info.image_bytes == image_bytes and info.num_chunks == len(cmap) and info.workspace_bytes == len(cmap) * 8
    ar.put(h_plan, image.view(np.uint8)[:image_bytes])
    if coef is not None:
        ar.put(h_coef, np.array([coef], dtype))
    if state is not None:
        raw = np.zeros(3, np.float64)
        raw.view(np.int64)[0] = state[0]
        raw[1:] = state[1:]
        ar.put(h_state, raw)
    ar.upload()
    d = N.SgwAdamStepDesc()
    d.plan, d.plan_bytes = ar.ptr(h_plan), image_bytes
    d.clip_coef = ar.ptr(h_coef) if clip_mode == AC.CLIP_COEF else None
    d.step_state = ar.ptr(h_state) if state is not None else None
    d.out_norm, d.workspace, d.workspace_bytes = ar.ptr(h_norm), ar.ptr(h_ws), len(cmap) * 8
    d.num_tensors, d.num_chunks = T, len(cmap)
    d.max_norm, d.beta1, d.beta2, d.eps, d.tau = max_norm, beta1, beta2, eps, tau
    d.dtype, d.clip_mode = N.POLICY_F64 if dtype == np.float64 else N.POLICY_F32, clip_mode
    d.flags = N.ADAM_ZERO_GRADS if zero_grads else 0
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for i in range(calls):
        d.step = 0 if state is not None else step + i
        N.check(lib.sgw_adam_step(C.byref(d), stream))
    ar.download()
    out = []
    for t, h in zip(tensors, handles):
        out.append({k: (ar.get(h[k], dtype, t[k].shape) if k in h else None) for k in ("p", "g", "m", "v", "t")})
    norm = ar.get(h_norm, np.float64, (2,))
    new_state = None
    if state is not None:
        raw = ar.get(h_state, np.float64, (3,))
        new_state = (int(raw.view(np.int64)[0]), float(raw[1]), float(raw[2]))
    return dict(tensors=out, norm=float(norm[0]), c=dtype.type(norm[1]), state=new_state)


def same(got, want, what, ctx=""):
    """Bit for bit; where the restatement has a NaN, any NaN (its sign and payload are the platform's)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (ctx, what)
    ok = (AC.bits(got) == AC.bits(want)) | (np.isnan(got) & np.isnan(want))
    assert ok.all(), f"{ctx} {what}: {int((~ok).sum())} of {ok.size} elements differ; the first at {np.argwhere(~ok)[0].tolist()}: " \
                     f"{got[~ok][0]!r} != {want[~ok][0]!r}"


def compare(got, want, ctx):
    for k, (a, b) in enumerate(zip(got["tensors"], want["tensors"])):
        for key in ("p", "g", "m", "v", "t"):
            assert (a[key] is None) == (b[key] is None)
            if a[key] is not None:
                same(a[key], b[key], f"tensor {k} {key}", ctx)
    same(np.float64(got["norm"]), np.float64(want["norm"]), "norm", ctx)
    same(got["c"], want["c"], "c", ctx)
    assert got["state"] == want["state"], (ctx, got["state"], want["state"])


def share(got, want, tol, what, ctx):
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    part = float(np.max(err / np.maximum(tol, 1e-300))) if np.size(err) else 0.0
    print(f"{ctx} {what}: {part:.4f} of the tolerance")
    assert part <= 1.0, (ctx, what, part)


def hyper(meta):
    return dict(beta1=meta["betas"][0], beta2=meta["betas"][1], eps=meta["eps"], tau=meta["tau"] or 0.0)


# ------------------------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("name", sorted(FIX))
def test_the_fixture_through_the_abi(built, name):
    meta, steps = FIX[name]["meta"], FIX[name]["steps"]
    dtype, clipped = np.dtype(meta["dtype"]), meta["max_norm"] is not None
    for s, rec in enumerate(steps):
        ctx = f"{name} step {s}"
        tensors = AC.fixture_tensors(rec, meta["lrs"], clipped)
        kw = dict(step=s + 1, **hyper(meta))
        if clipped:                                     # the reference's own coefficient fed in: its moments and targets bit for bit
            kw.update(clip_mode=AC.CLIP_COEF, coef=AC.torch_clip_coef(rec["norm"], meta["max_norm"], dtype))
        got = run_abi(tensors, dtype, **kw)
        compare(got, AC.restate(tensors, dtype, **kw), ctx)
        for k, t in enumerate(got["tensors"]):
            AC.same_bits(t["m"], rec["exp_avg_after"][k], f"exp_avg {k}", ctx)
            AC.same_bits(t["v"], rec["exp_avg_sq_after"][k], f"exp_avg_sq {k}", ctx)
            if clipped:
                AC.same_bits(t["t"], rec["target_after"][k], f"target {k}", ctx)
            share(t["p"], rec["param_after"][k], AC.param_tolerance(rec["param_after"][k], rec["param_before"][k], dtype), f"param {k}", ctx)
        if clipped:                                     # the kernel's own norm: only the norm is compared with the reference
            kw = dict(step=s + 1, clip_mode=AC.CLIP_NORM, max_norm=meta["max_norm"], **hyper(meta))
            got = run_abi(tensors, dtype, **kw)
            compare(got, AC.restate(tensors, dtype, **kw), ctx + " NORM")
            n_total = sum(g.size for g in rec["grad"])
            share(got["norm"], float(rec["norm"]), AC.norm_tolerance(n_total, got["norm"], dtype), "norm", ctx)
            assert (got["c"] < 1) == (float(rec["norm"]) > 1)


@pytest.mark.parametrize("name", sorted(FIX))
def test_the_fixture_through_fused_adam(built, name):
    meta, steps = FIX[name]["meta"], FIX[name]["steps"]
    dtype, clipped = np.dtype(meta["dtype"]), meta["max_norm"] is not None
    params = [torch.nn.Parameter(torch.from_numpy(a.copy()).cuda()) for a in steps[0]["param_before"]]
    targets = [torch.from_numpy(a.copy()).cuda() for a in steps[0]["target_before"]] if clipped else None
    lrs = meta["lrs"]
    groups = [dict(params=[p for p, lr in zip(params, lrs) if lr == value], lr=value) for value in dict.fromkeys(lrs)]
    opt = optim.FusedAdam(groups, betas=tuple(meta["betas"]), eps=meta["eps"], max_grad_norm=meta["max_norm"], target_params=targets, tau=meta["tau"])
    state = AC.fixture_tensors(steps[0], lrs, clipped)
    for p in params:
        p.grad = torch.zeros_like(p)
    tables = None
    for s, rec in enumerate(steps):
        ctx = f"{name} step {s}"
        for k, p in enumerate(params):
            p.grad.copy_(torch.from_numpy(rec["grad"][k]))
            state[k]["g"] = rec["grad"][k]
        norm = opt.step()
        want = AC.restate(state, dtype, clip_mode=AC.CLIP_NORM if clipped else AC.CLIP_NONE, max_norm=meta["max_norm"] or 0.0, step=s + 1, **hyper(meta))
        for k, p in enumerate(params):
            same(p.detach().cpu().numpy(), want["tensors"][k]["p"], f"param {k}", ctx)
            same(opt.state[p]["exp_avg"].cpu().numpy(), want["tensors"][k]["m"], f"exp_avg {k}", ctx)
            same(opt.state[p]["exp_avg_sq"].cpu().numpy(), want["tensors"][k]["v"], f"exp_avg_sq {k}", ctx)
            same(p.grad.cpu().numpy(), rec["grad"][k], f"grad {k} (not written back)", ctx)
            if clipped:
                same(targets[k].cpu().numpy(), want["tensors"][k]["t"], f"target {k}", ctx)
        if clipped:
            assert norm.dtype == torch.float64 and norm.dim() == 0 and float(norm) == want["norm"]
            share(float(norm), float(rec["norm"]), AC.norm_tolerance(sum(g.size for g in rec["grad"]), float(norm), dtype), "norm", ctx)
        else:
            assert norm is None
        state = want["tensors"]
        assert tables is None or all(a is b for a, b in zip(tables, opt._tables))          # stable pointers: one plan, one upload
        tables = list(opt._tables)
        assert len(tables) == 1
    sd = opt.state_dict()
    assert all(float(v["step"]) == len(steps) for v in sd["state"].values()) and len(sd["state"]) == len(params)


# ------------------------------------------------------------------------------------------------------------- shapes, modes, alignment
@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "one element off 16 bytes"])
@pytest.mark.parametrize("clip_mode", [AC.CLIP_NONE, AC.CLIP_NORM, AC.CLIP_COEF], ids=["NONE", "NORM", "COEF"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_every_numel_mode_and_alignment(built, dtype, clip_mode, misalign):
    numels = NUMELS + (0, 7)
    tensors = make(numels, dtype, seed=3, skip=(3, 11), no_target=(1, 4, 6, 8))       # a NULL grad, a zero-numel tensor, soft update on and off
    kw = dict(clip_mode=clip_mode, max_norm=1.0, coef=0.3 if clip_mode == AC.CLIP_COEF else None, tau=0.01, step=2,
              zero_grads=bool(misalign) != (dtype == np.float64))
    got = run_abi(tensors, dtype, misalign=misalign, **kw)
    want = AC.restate(tensors, dtype, **kw)
    compare(got, want, f"{np.dtype(dtype).name} mode {clip_mode} misalign {misalign}")
    assert clip_mode != AC.CLIP_NORM or (want["norm"] > 1 and want["c"] < 1)
    same(got["tensors"][3]["p"], tensors[3]["p"], "a skipped tensor's param")
    same(got["tensors"][3]["t"], tensors[3]["t"], "a skipped tensor's target")


@pytest.mark.parametrize("what", ["below max_norm", "exactly 0", "inf gradient", "NaN gradient"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_norm_below_zero_and_not_finite(built, dtype, what):
    tensors = make((5, 4097, 33), dtype, seed=9, scale=1e-4)
    if what == "exactly 0":
        for t in tensors:
            t["g"][:] = 0
    elif what == "inf gradient":
        tensors[1]["g"][4096] = np.inf
    elif what == "NaN gradient":
        tensors[2]["g"][7] = np.nan
    kw = dict(clip_mode=AC.CLIP_NORM, max_norm=1.0, tau=0.5, step=1)
    got, want = run_abi(tensors, dtype, **kw), AC.restate(tensors, dtype, **kw)
    compare(got, want, what)
    if what in ("below max_norm", "exactly 0"):
        assert got["c"] == 1 and (got["norm"] == 0) == (what == "exactly 0")
    elif what == "inf gradient":
        assert got["norm"] == np.inf and got["c"] == 0 and np.isnan(got["tensors"][1]["p"][4096]) and not np.isnan(got["tensors"][0]["p"]).any()
    else:
        assert np.isnan(got["norm"]) and np.isnan(got["c"]) and all(np.isnan(t["p"]).all() for t in got["tensors"])


@pytest.mark.parametrize("count", [1, 17, 300])
def test_tensor_counts(built, count):
    rng = np.random.default_rng(count)
    numels = [int(n) for n in rng.integers(1, 40, size=count)]
    tensors = make(numels, np.float32, seed=count, skip=(5,) if count > 5 else ())
    kw = dict(clip_mode=AC.CLIP_NORM, max_norm=2.0, tau=0.1, step=3, zero_grads=True)
    compare(run_abi(tensors, np.float32, **kw), AC.restate(tensors, np.float32, **kw), f"{count} tensors")


def test_the_device_step_state_through_the_abi(built):
    tensors = make((5, 4097), np.float64, seed=21)
    kw = dict(clip_mode=AC.CLIP_NORM, max_norm=1.0, tau=0.1)
    got = run_abi(tensors, np.float64, state=AC.fresh_state(), calls=3, **kw)
    want, state = dict(tensors=tensors), AC.fresh_state()
    for _ in range(3):
        want = AC.restate(want["tensors"], np.float64, state=state, **kw)
        state = want["state"]
    assert state[0] == 3 and state[1] == 0.9 * 0.9 * 0.9
    compare(got, want, "three calls on a device state")
    # ... and without a norm launch A only advances the state
    kw = dict(clip_mode=AC.CLIP_NONE, tau=0.1)
    compare(run_abi(tensors, np.float64, state=(6, 0.5, 0.99), **kw), AC.restate(tensors, np.float64, state=(6, 0.5, 0.99), **kw), "NONE on a device state")


def test_2049_chunks_twice_the_same_bits(built):
    n = 2049 * AC.CHUNK
    gen = torch.Generator(device="cuda").manual_seed(5)
    start = [torch.randn(n, device="cuda", generator=gen) for _ in range(2)] + [torch.rand(n, device="cuda", generator=gen) * 0.01]
    g = torch.randn(n, device="cuda", generator=gen)
    runs = []
    for _ in range(2):
        p = torch.nn.Parameter(start[0].clone())
        p.grad = g.clone()
        opt = optim.FusedAdam([p], max_grad_norm=1.0)
        opt.state[p] = dict(step=torch.tensor(4.0), exp_avg=start[1].clone(), exp_avg_sq=start[2].clone())
        norm = opt.step()
        assert opt._tables[0].desc.num_chunks == 2049 > AC.MAX_BLOCKS
        runs.append((p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], norm.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int64),
                           b.view(torch.int32) if b.dtype == torch.float32 else b.view(torch.int64))
    g_host = g.cpu().numpy()
    assert float(runs[0][3]) == AC.grad_norm([g_host])                            # the norm's order does not depend on the grid
    c = AC.clip_coef(float(runs[0][3]), 1.0, np.float32)
    head = AC.restate([dict(p=start[0][:4096].cpu().numpy(), g=g_host[:4096], m=start[1][:4096].cpu().numpy(), v=start[2][:4096].cpu().numpy(),
                            t=None, lr=1e-3)], np.float32, clip_mode=AC.CLIP_COEF, coef=c, step=5)
    same(runs[0][0][:4096].cpu().numpy(), head["tensors"][0]["p"], "the first chunk's params")
    tail = AC.restate([dict(p=start[0][-4096:].cpu().numpy(), g=g_host[-4096:], m=start[1][-4096:].cpu().numpy(), v=start[2][-4096:].cpu().numpy(),
                            t=None, lr=1e-3)], np.float32, clip_mode=AC.CLIP_COEF, coef=c, step=5)
    same(runs[0][0][-4096:].cpu().numpy(), tail["tensors"][0]["p"], "the last chunk's params (the strided workgroup's)")


# ------------------------------------------------------------------------------------------------------------- recording
def test_three_device_steps_equal_three_replays_of_one_capture(built):
    rng = np.random.default_rng(17)
    shapes = [(33, 7), (7,), (4097,)]
    grads = [[rng.normal(size=s).astype(np.float32) for s in shapes] for _ in range(4)]
    init = [rng.normal(size=s).astype(np.float32) for s in shapes]

    def fresh():
        params = [torch.nn.Parameter(torch.from_numpy(a.copy()).cuda()) for a in init]
        targets = [torch.zeros_like(p) for p in params]
        for p, g in zip(params, grads[0]):
            p.grad = torch.from_numpy(g.copy()).cuda()
        opt = optim.FusedAdam(params, lr=1e-2, max_grad_norm=1.0, target_params=targets, tau=0.05, device_step=True)
        opt.step()                                       # builds and uploads the table; step 1
        return params, targets, opt

    def load(params, i):
        for p, g in zip(params, grads[i]):
            p.grad.copy_(torch.from_numpy(g))

    eager, eager_t, opt_e = fresh()
    for i in (1, 2, 3):
        load(eager, i)
        opt_e.step()
    rec, rec_t, opt_r = fresh()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt_r.step()
    for i in (1, 2, 3):
        load(rec, i)
        graph.replay()
    torch.cuda.synchronize()
    want, state = dict(tensors=[dict(p=a, g=None, m=np.zeros_like(a), v=np.zeros_like(a), t=np.zeros_like(a), lr=1e-2) for a in init]), AC.fresh_state()
    for i in range(4):
        for t, g in zip(want["tensors"], grads[i]):
            t["g"] = g
        want = AC.restate(want["tensors"], np.float32, clip_mode=AC.CLIP_NORM, max_norm=1.0, tau=0.05, state=state)
        state = want["state"]
    for k in range(len(shapes)):
        same(eager[k].detach().cpu().numpy(), want["tensors"][k]["p"], f"eager param {k}")
        same(rec[k].detach().cpu().numpy(), want["tensors"][k]["p"], f"replayed param {k}")
        same(rec_t[k].cpu().numpy(), want["tensors"][k]["t"], f"replayed target {k}")
        same(eager_t[k].cpu().numpy(), want["tensors"][k]["t"], f"eager target {k}")
        same(opt_r.state[rec[k]]["exp_avg_sq"].cpu().numpy(), want["tensors"][k]["v"], f"replayed exp_avg_sq {k}")
    assert all(float(v["step"]) == 4.0 for v in opt_r.state_dict()["state"].values())     # read back from the device: replays are counted
    assert all(float(v["step"]) == 4.0 for v in opt_e.state_dict()["state"].values())
    # against a step passed by value: inside device_step_tolerance, summed over the steps taken (the gradients do not depend on the
    # parameters here, so the moments are the same and each step adds its own difference to what the parameters carry already)
    by_value = dict(tensors=[dict(p=a, g=None, m=np.zeros_like(a), v=np.zeros_like(a), t=np.zeros_like(a), lr=1e-2) for a in init])
    budget = [np.zeros(s) for s in shapes]
    for i in range(4):
        for t, g in zip(by_value["tensors"], grads[i]):
            t["g"] = g
        before = [t["p"] for t in by_value["tensors"]]
        by_value = AC.restate(by_value["tensors"], np.float32, clip_mode=AC.CLIP_NORM, max_norm=1.0, tau=0.05, step=i + 1)
        budget = [b + AC.device_step_tolerance(t["p"], p0, i + 1, np.float32) for b, t, p0 in zip(budget, by_value["tensors"], before)]
    for k in range(len(shapes)):
        share(eager[k].detach().cpu().numpy(), by_value["tensors"][k]["p"], budget[k], f"param {k}", "device state against by value, 4 steps")


def test_a_linear_trained_three_steps_against_torch_adam_on_a_cpu_copy(built):
    """The loss is linear in the parameters and every value dyadic, so the CPU's and the device's gradients are the same numbers; what
    differs is Adam's arithmetic alone.  The moments are the same bits; the parameters may part by ``param_tolerance`` per step, summed
    over the steps taken (each step starts from the other's parameters within the bound so far and adds its own two roundings)."""
    torch.manual_seed(3)
    cpu = torch.nn.Linear(6, 4)
    with torch.no_grad():
        for p in cpu.parameters():
            p.copy_(torch.round(p * 64) / 64)
    dev = torch.nn.Linear(6, 4).cuda()
    dev.load_state_dict(cpu.state_dict())
    theirs = torch.optim.Adam(cpu.parameters(), lr=1e-2)
    ours = optim.FusedAdam(dev.parameters(), lr=1e-2, zero_grads=True)
    rng = np.random.default_rng(2)
    budget = [np.zeros(tuple(p.shape)) for p in cpu.parameters()]
    for s in range(3):
        x = torch.from_numpy(rng.integers(-4, 5, size=(8, 6)).astype(np.float32))
        w = torch.from_numpy(rng.integers(-2, 3, size=(8, 4)).astype(np.float32) / 4)
        before = [p.detach().clone().numpy() for p in cpu.parameters()]
        theirs.zero_grad()
        (cpu(x) * w).sum().backward()
        theirs.step()
        (dev(x.cuda()) * w.cuda()).sum().backward()           # (zero_grads left +0 behind: backward accumulates into it)
        for p, q in zip(cpu.parameters(), dev.parameters()):
            assert torch.equal(p.grad, q.grad.cpu())
        ours.step()
        for k, (p, q) in enumerate(zip(cpu.parameters(), dev.parameters())):
            assert not q.grad.any()
            AC.same_bits(ours.state[q]["exp_avg"].cpu().numpy(), theirs.state[p]["exp_avg"].numpy(), f"exp_avg {k}", f"step {s}")
            AC.same_bits(ours.state[q]["exp_avg_sq"].cpu().numpy(), theirs.state[p]["exp_avg_sq"].numpy(), f"exp_avg_sq {k}", f"step {s}")
            budget[k] = budget[k] + AC.param_tolerance(p.detach().numpy(), before[k], np.float32)
            share(q.detach().cpu().numpy(), p.detach().numpy(), budget[k], f"param {k}", f"step {s}")
