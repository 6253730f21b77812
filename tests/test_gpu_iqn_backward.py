"""``sgw_iqn_backward`` on the device: EVERY output bit for bit against the NumPy restatement (``tests/iqn_backward_common.py``) fed the
kernel's own cos, over a pruned product of shapes around the tile sizes and the matrix pair's padding cases (n N = 1, 2, odd) with
float32 and uint8 states; each output NULL in turn, each pointer one element off a 16-byte boundary, a stride above D, guard bytes round
every output and the workspace, two calls with identical bits, a NaN that stays out of the other rows' ``out_grad_h``; the reference's
fixture (``tests/golden/iqn_backward``) through ``IQN.forward_fused`` + ``backward()`` under the cap ``d <= 4 d_ref + 2^-22 max|g64|``,
training mode's ``sigma_*`` gradients included; and one learner step at the reference's shape (``TurnBuffer.sample`` -> two
``quantiles`` -> ``forward_fused`` -> ``iqn_loss`` -> ``backward()`` -> ``FusedAdam.step()``) against the same step with ``IQN.forward``
and torch's autograd, both measured from the float64 step."""
import copy
import ctypes as C

import numpy as np
import pytest

from sorrel_amd import _native as N
from tests import iqn_backward_common as BC
from tests import iqn_forward_common as FC
from tests.gpu_common import torch_cuda  # noqa: F401
from tests.learner_common import DEV, Guarded

pytestmark = pytest.mark.gpu

CASES = BC.load_fixture()
OUTPUTS = FC.WEIGHTS + ("grad_h",)
INPUTS = FC.WEIGHTS + ("taus", "h", "grad_quantiles")


def abi_backward(torch, w, states, Nq, taus, grad, *, off=(), skip=(), stride=None, untouched=False):
    """``sgw_iqn_forward`` (which leaves ``h``) and one ``sgw_iqn_backward`` call over host arrays.  The inputs and outputs named in ``off``
    start one element past a 16-byte boundary; the outputs named in ``skip`` are NULL; ``stride``: the states' row stride in elements.
    Every output and the workspace sit inside guards, which must come back untouched.  Returns ``(dict of host arrays, cos)``."""
    lib = N.load()
    states = np.ascontiguousarray(states)
    B, D = states.shape
    L, A = np.asarray(w["w_ff"]).shape[0], np.asarray(w["w_adv"]).shape[0]
    stride = D if stride is None else stride
    padded = np.full((max(B, 1), stride), 77, states.dtype)
    padded[:B, :D] = states
    keep = {"states": torch.from_numpy(padded).to(DEV)}

    def device(name, a):
        flat = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), np.ascontiguousarray(a, np.float32).ravel(), np.zeros(1, np.float32)])).to(DEV)
        keep[name] = flat[1:] if name in off else flat[1:].clone()
        assert name not in off or keep[name].data_ptr() % 16 == 4
        return keep[name].data_ptr()

    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = N.SgwIqnForwardDesc()
    b = N.SgwIqnBackwardDesc()
    for d in (f, b):
        d.states = keep["states"].data_ptr()
        for name in FC.WEIGHTS:
            setattr(d, name, device(name, w[name]) if d is f else keep[name].data_ptr())
        d.n, d.state_stride = B, stride
        d.in_features, d.layer_size, d.num_quantiles, d.num_actions, d.n_cos = D, L, Nq, A, FC.N_COS
        d.state_type = 1 if states.dtype == np.uint8 else 0
    f.taus = b.taus = device("taus", np.asarray(taus, np.float32).reshape(B, Nq))
    quant = torch.empty((max(B * Nq * A, 1),), dtype=torch.float32, device=DEV)
    cos = torch.empty((max(B * Nq * FC.N_COS, 1),), dtype=torch.float32, device=DEV)
    h = torch.zeros((B * L + 2,), dtype=torch.float32, device=DEV)[1:]
    keep["h"] = h if "h" in off else h.clone()
    f.out_quantiles, f.out_cos = quant.data_ptr(), cos.data_ptr()
    f.workspace, f.workspace_bytes = keep["h"].data_ptr(), B * L * 4
    assert lib.sgw_iqn_forward(C.byref(f), stream) == N.OK, lib.sgw_last_error()
    b.h = keep["h"].data_ptr()
    b.grad_quantiles = device("grad_quantiles", np.asarray(grad, np.float32).reshape(B, Nq, A))
    shapes = {k: np.asarray(w[k]).shape for k in FC.WEIGHTS}
    shapes["grad_h"] = (B, L)
    outs = {k: (None if k in skip else Guarded(torch, shapes[k], np.float32, shift=4 if k in off else 0)) for k in OUTPUTS}
    for k in FC.WEIGHTS:
        setattr(b, "out_" + k, outs[k].ptr if outs[k] else None)
    b.out_grad_h = outs["grad_h"].ptr if outs["grad_h"] else None
    need = int(lib.sgw_iqn_backward_workspace_bytes(B, D, L, Nq, A))
    assert need == 4 * (B * Nq * (4 * L + 64 + A + 1) + B * L)
    ws = Guarded(torch, need // 4, np.float32, shift=4 if "workspace" in off else 0)
    b.workspace, b.workspace_bytes = ws.ptr, need
    assert lib.sgw_iqn_backward(C.byref(b), stream) == N.OK, lib.sgw_last_error()
    torch.cuda.synchronize()
    for g in list(outs.values()) + [ws]:
        assert g is None or g.intact(), "bytes outside an output were written"
    if untouched:
        assert all(g is None or (g.numpy().view(np.uint8) == 0xA5).all() for g in list(outs.values()) + [ws])
    return {k: (outs[k].numpy() if outs[k] else None) for k in OUTPUTS}, cos[:B * Nq * FC.N_COS].cpu().numpy().reshape(B, Nq, FC.N_COS)


def check_bits(got, cos, w, states, grad, ctx):
    want = BC.restate(w, states, cos, grad)
    for k in OUTPUTS:
        if got[k] is not None:
            FC.same_bits(got[k], want[k].reshape(got[k].shape), k, ctx)


# ------------------------------------------------------------------------------------------------------------- 1: shapes
# (L, D, N, A, rows): every value of an axis meets small and large values of the others; rows N L^2 <= 2^24.  N = 1 with 1, 2, 7, 9, 65 and
# 257 rows gives n N = 1, 2 and odd values: the matrix pair's padding cases
SHAPES = [
    (1, 1, 1, 1, 1), (1, 875, 64, 64, 257), (1, 63, 12, 5, 9), (1, 65, 2, 4, 65), (1, 65, 13, 64, 7), (1, 63, 1, 4, 2),
    (31, 63, 13, 64, 7), (31, 1, 1, 4, 257), (31, 875, 2, 1, 2), (31, 65, 64, 4, 9), (31, 63, 12, 64, 1), (31, 65, 2, 5, 65),
    (32, 63, 12, 4, 65), (32, 1, 64, 64, 1), (32, 65, 1, 5, 257), (32, 875, 13, 4, 7), (32, 1, 2, 64, 9), (32, 63, 12, 1, 2),
    (33, 65, 13, 5, 9), (33, 1, 2, 64, 257), (33, 63, 64, 1, 65), (33, 875, 12, 4, 2), (33, 63, 1, 5, 7), (33, 65, 13, 64, 1),
    (250, 875, 12, 4, 2), (250, 1, 1, 1, 257), (250, 63, 64, 64, 1), (250, 65, 2, 64, 65), (250, 63, 13, 5, 7), (250, 65, 12, 4, 9),
    (256, 875, 1, 64, 9), (256, 63, 64, 1, 1), (256, 1, 13, 4, 2), (256, 65, 2, 5, 65), (256, 1, 12, 64, 7), (256, 63, 2, 4, 1),
    (250, 875, 12, 4, 7), (5, 7, 2, 3, 9), (96, 65, 5, 4, 65), (224, 64, 12, 5, 9),
]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(str(v) for v in s) for s in SHAPES])
def test_shapes_bit_for_bit(torch_cuda, shape):
    L, D, Nq, A, B = shape
    assert B * Nq * L * L <= 1 << 24
    rng = np.random.default_rng(sum(v * 1000 ** i for i, v in enumerate(shape)) & 0xFFFFFFFF)
    w = FC.random_weights(rng, D, L, A)
    taus = rng.random(size=(B, Nq)).astype(np.float32)
    grad = rng.normal(size=(B, Nq, A)).astype(np.float32)
    for x in (rng.normal(size=(B, D)).astype(np.float32), (rng.random(size=(B, D)) < 0.3).astype(np.uint8) * rng.integers(1, 256, size=(B, D)).astype(np.uint8)):
        got, cos = abi_backward(torch_cuda, w, x, Nq, taus, grad)
        check_bits(got, cos, w, x, grad, f"{shape} {x.dtype}")


# ------------------------------------------------------------------------------------------------------------- 2: the call
def test_strides_alignment_optional_outputs_guards_and_determinism(torch_cuda):
    rng = np.random.default_rng(21)
    D, L, Nq, A, B = 65, 33, 13, 5, 9
    w = FC.random_weights(rng, D, L, A)
    x = rng.normal(size=(B, D)).astype(np.float32)
    taus = rng.random(size=(B, Nq)).astype(np.float32)
    grad = rng.normal(size=(B, Nq, A)).astype(np.float32)
    base, cos = abi_backward(torch_cuda, w, x, Nq, taus, grad)
    check_bits(base, cos, w, x, grad, "base")

    def same(got, ctx):
        for k in OUTPUTS:
            if got[k] is not None:
                FC.same_bits(got[k], base[k], k, ctx)

    same(abi_backward(torch_cuda, w, x, Nq, taus, grad)[0], "twice")
    same(abi_backward(torch_cuda, w, x, Nq, taus, grad, stride=D + 7)[0], "a state_stride above D")
    same(abi_backward(torch_cuda, w, x, Nq, taus, grad, stride=D + 1)[0], "an odd state_stride")
    for name in INPUTS + OUTPUTS + ("workspace",):
        same(abi_backward(torch_cuda, w, x, Nq, taus, grad, off=(name,))[0], f"{name} one element off a 16-byte boundary")
    same(abi_backward(torch_cuda, w, x, Nq, taus, grad, off=INPUTS + OUTPUTS + ("workspace",))[0], "everything off")
    for name in OUTPUTS:
        got = abi_backward(torch_cuda, w, x, Nq, taus, grad, skip=(name,))[0]
        assert got[name] is None
        same(got, f"{name} is NULL")
    same(abi_backward(torch_cuda, w, x, Nq, taus, grad, skip=tuple(k for k in OUTPUTS if k != "b_ff"))[0], "one bias alone")
    same(abi_backward(torch_cuda, w, x, Nq, taus, grad, skip=OUTPUTS[:-1])[0], "grad_h alone")
    abi_backward(torch_cuda, w, x[:0], Nq, taus[:0], grad[:0], untouched=True)     # n == 0 launches nothing and writes nothing


def test_a_nan_stays_out_of_the_other_rows_grad_h(torch_cuda):
    rng = np.random.default_rng(22)
    D, L, Nq, A, B = 7, 33, 12, 4, 11
    w = FC.random_weights(rng, D, L, A)
    x = rng.normal(size=(B, D)).astype(np.float32)
    taus = rng.random(size=(B, Nq)).astype(np.float32)
    grad = rng.normal(size=(B, Nq, A)).astype(np.float32)
    clean, _ = abi_backward(torch_cuda, w, x, Nq, taus, grad)
    x2 = x.copy()
    x2[6, 3] = np.nan
    got, cos = abi_backward(torch_cuda, w, x2, Nq, taus, grad)
    others = np.arange(B) != 6
    FC.same_bits(got["grad_h"][others], clean["grad_h"][others], "grad_h", "the rows beside the NaN")
    check_bits(got, cos, w, x2, grad, "with a NaN")
    assert np.isnan(got["w_ff"]).any() and np.isnan(got["w_head"][:, 3]).all()   # it reaches the weight gradients, as IEEE says
    x3 = x.copy()
    x3[2, 0] = np.inf
    got, cos = abi_backward(torch_cuda, w, x3, Nq, taus, grad)
    check_bits(got, cos, w, x3, grad, "with an infinity")


# ------------------------------------------------------------------------------------------------------------- 3: the reference
def to_net(torch, c):
    from sorrel_amd.models import iqn as M

    net = M.IQN((c["D"],), c["A"], c["L"], seed=0, n_quantiles=c["N"], n_frames=1)
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in c["sd"].items()})
    net.train(bool(c["train"]))
    return net.to(DEV)


@pytest.mark.parametrize("tag", sorted(CASES))
def test_fixture_through_forward_fused_and_backward(torch_cuda, tag, monkeypatch):
    torch = torch_cuda
    c = CASES[tag]
    net = to_net(torch, c)
    monkeypatch.setattr(torch.Tensor, "normal_", lambda t, *a, **k: t)           # training mode applies the fixture's noise
    quant, taus = net.forward_fused(torch.from_numpy(c["states"]).to(DEV), taus=torch.from_numpy(c["taus"]).to(DEV))
    monkeypatch.undo()
    assert quant.requires_grad and tuple(quant.shape) == (c["B"], c["N"], c["A"]) and torch.equal(taus.cpu(), torch.from_numpy(c["taus"]))
    plain = net.quantiles(torch.from_numpy(c["states"]).to(DEV), taus=torch.from_numpy(c["taus"]).to(DEV)) if not c["train"] else None
    assert plain is None or torch.equal(plain.quantiles, quant.detach())
    (quant * torch.from_numpy(c["grad"]).to(DEV)).sum().backward()
    got = {k: p.grad.cpu().numpy() for k, p in net.named_parameters() if p.grad is not None}
    assert sorted(got) == sorted(c["g64"])
    for k in sorted(got):
        g64 = c["g64"][k]
        d = BC.distance(BC.kept(k, got[k], c), g64)
        print(f"{tag} {k}: d_ref {c['d_ref'][k]:.3e}, d {d:.3e}, cap {BC.cap(c['d_ref'][k], g64):.3e}")
        assert d <= BC.cap(c["d_ref"][k], g64), (tag, k, d, c["d_ref"][k])


# ------------------------------------------------------------------------------------------------------------- 4: one learner step
def test_one_learner_step_at_the_reference_shape(torch_cuda, monkeypatch):
    torch = torch_cuda
    from sorrel_amd import losses
    from sorrel_amd.buffers import TurnBuffer
    from sorrel_amd.models import iqn as M
    from sorrel_amd.optim import FusedAdam

    s = FC.load_fixture()[BC.BIG_TAG]
    D, L, Nq, A, B, frames = s["D"], s["L"], s["N"], s["A"], 64, 5
    rng = np.random.default_rng(23)
    ring = TurnBuffer(24, 8, (1, 7, 5, 5), device=DEV, obs_dtype=torch.uint8)
    ring.obs.copy_(torch.from_numpy((rng.random(size=tuple(ring.obs.shape)) < 0.15).astype(np.uint8)))
    ring.actions.copy_(torch.from_numpy(rng.integers(0, A, size=tuple(ring.actions.shape)).astype(np.uint8)))
    ring.rewards.copy_(torch.from_numpy(rng.normal(size=tuple(ring.rewards.shape)).astype(np.float32)))
    ring.size = ring.capacity
    starts, envs = rng.integers(0, 24 - frames - 1, size=B).tolist(), rng.integers(0, 8, size=B).tolist()
    states, actions, rewards, next_states, dones, valid = ring.sample(B, agent=0, n_frames=frames, starts=starts, envs=envs)
    assert tuple(states.reshape(B, -1).shape) == (B, D)
    t0, t1, t2 = (torch.from_numpy(rng.random(size=(B, Nq)).astype(np.float32)).to(DEV) for _ in range(3))
    discount, lr = 0.99 ** 3, 2.5e-4

    def nets():
        local = M.IQN((D,), A, L, seed=0, n_quantiles=Nq, n_frames=1)
        local.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in s["sd"].items()})
        target = copy.deepcopy(local)
        with torch.no_grad():
            for p in target.parameters():
                p.mul_(0.75)
        return local.to(DEV).train(True), target.to(DEV).train(False)

    monkeypatch.setattr(torch.Tensor, "normal_", lambda t, *a, **k: t)           # every call applies the fixture's noise
    after = {}
    for fused in (True, False):
        local, target = nets()
        opt = FusedAdam(local.parameters(), lr=lr, max_grad_norm=1.0, target_params=list(target.parameters()), tau=1e-3)
        qnl = local.quantiles(next_states, taus=t1).quantiles
        qnt = target.quantiles(next_states, taus=t2).quantiles
        if fused:
            q, taus = local.forward_fused(states, taus=t0)
        else:
            with monkeypatch.context() as mp:
                mp.setattr(torch, "rand", lambda *shape, **kw: t0.cpu().reshape(shape))
                q, taus = local(states.reshape(B, -1).float(), Nq)
        loss = losses.iqn_loss(q, taus, qnl, qnt, actions, rewards, dones, valid, discount)
        opt.zero_grad()
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        after[fused] = {k: p.detach().cpu().numpy() for k, p in local.named_parameters()}
        if fused:
            shared = (qnl.double(), qnt.double())
    # the float64 step: the same next-state quantiles, the network, the loss, the clipping and Adam in float64 by torch ops
    local, _ = nets()
    local = local.double()
    c64 = torch.cos(t0.double().reshape(B, Nq, 1) * local.pis)
    local.calc_cos = lambda batch_size, n_tau=8: (c64, t0.double().reshape(B, Nq, 1))
    q, taus = local(states.reshape(B, -1).double(), Nq)
    loss = losses._iqn_loss_torch(q, taus, shared[0], shared[1], actions, rewards.double(), dones.double(), valid.double(), discount)[0]
    loss.backward()
    torch.nn.utils.clip_grad_norm_(local.parameters(), 1.0)
    torch.optim.Adam(local.parameters(), lr=lr).step()
    monkeypatch.undo()
    before = {k: np.array(v) for k, v in s["sd"].items()}
    for k, p in local.named_parameters():
        p64 = p.detach().cpu().numpy()
        d_ref, d = BC.distance(after[False][k], p64), BC.distance(after[True][k], p64)
        print(f"{k}: d_ref {d_ref:.3e}, d {d:.3e}, cap {BC.cap(d_ref, p64):.3e}")
        assert not np.array_equal(after[True][k], before[k]), k                  # (the step moved it)
        assert d <= BC.cap(d_ref, p64), (k, d, d_ref)
