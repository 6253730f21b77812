"""``sgw_ppo_loss`` on the device: the reference's fixture (``tests/golden/ppo_loss``) through the C ABI and through both Python entry
points, in float64 and as float32 casts; a grid of action counts (every bucket and the generic loop), row counts around the wave and the
tile, both modes, strides, a base the 16-byte accesses must step aside for, both action types, both value / return types, ``entropy_coef``
0 and ``eps_clip`` 0 -- all against the NumPy restatement (``tests/ppo_loss_common.py``, itself pinned by the fixture in
``tests/test_ppo_loss_cpu.py``); more row tiles than workgroups; two runs with identical bits; invalid rows and the bytes around every
output and the workspace; NULL optional outputs; ``ppo_loss(...).backward()``; a replayed capture; and one end-to-end step of a
four-layer actor and critic against the reference's parameter gradients.

Bounds.  Every comparison uses the tolerance FORMULAS of ``tests/ppo_loss_common.py``, evaluated on the restatement's intermediates; a
float32 output is the restatement's float64 value rounded once, and may sit one float32 step away where the two float64 values straddle
a rounding boundary (``f32_slack``).  Which branch a row takes is not a matter of tolerance: every case asserts ON THE RESTATEMENT that
ratios, surrogates and probabilities keep 2^-40 from every threshold.  No expectation comes from the kernel."""
import ctypes as C

import numpy as np
import pytest

from sorrel_amd import _native as N
from tests import ppo_loss_common as LC
from tests.gpu_common import torch_cuda  # noqa: F401
from tests.learner_common import DEV, Guarded

pytestmark = pytest.mark.gpu

SETS, E2E = LC.load_fixture()


def abi_loss(torch, x, values, actions, old, returns, eps_clip, c, vc=0.5, *, logits=False, stride=None, misalign=False, want_gd=True, want_gv=True,
             want_rows=True, grad_off=False):
    """One ``sgw_ppo_loss`` call over host arrays laid out as the caller describes; every output and the workspace sit inside guards, which
    must come back untouched, as must what lies between the rows of the gradient.  Returns a dict of host arrays."""
    lib = N.load()
    n, na = x.shape
    stride = na if stride is None else stride
    host = np.full((n, stride), 0.015625, x.dtype)             # (what lies between the rows is a valid weight: reading it would change results)
    host[:, :na] = x
    flat = torch.from_numpy(np.concatenate([np.zeros(1, x.dtype), host.ravel()])).to(DEV)
    dist = flat[1:] if misalign else flat[1:].clone()
    assert not misalign or dist.data_ptr() % 16 == x.dtype.itemsize          # (the 16-byte accesses must step aside)
    keep = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (values, actions, old, returns)]
    off = 1 if grad_off else 0                                   # the gradient's base one element past a 16-byte boundary, dist's on one
    gd = Guarded(torch, n * stride + off, x.dtype) if want_gd else None
    gv = Guarded(torch, n, values.dtype) if want_gv else None
    rows = Guarded(torch, 3 * n, np.float64) if want_rows else None
    terms = Guarded(torch, 4, np.float64)
    need = int(lib.sgw_ppo_loss_workspace_bytes(n))
    assert need == min((n + 255) // 256, LC.max_blocks()) * 24
    ws = Guarded(torch, need // 8, np.float64)
    d = N.SgwPpoLossDesc()
    d.dist = dist.data_ptr()
    d.values, d.actions, d.old_log_probs, d.returns = (t.data_ptr() for t in keep)
    d.out_grad_dist, d.out_grad_values, d.out_row_terms = (g.ptr if g else None for g in (gd, gv, rows))
    if gd and off:
        d.out_grad_dist = gd.ptr + x.dtype.itemsize
        assert dist.data_ptr() % 16 == 0 and d.out_grad_dist % 16 == x.dtype.itemsize
    d.out_terms, d.workspace, d.workspace_bytes = terms.ptr, ws.ptr, need
    d.n, d.row_stride, d.num_actions = n, stride, na
    d.eps_clip, d.entropy_coef, d.value_coef = eps_clip, c, vc
    f = {np.dtype(np.float32): N.POLICY_F32, np.dtype(np.float64): N.POLICY_F64}
    d.dist_type, d.mode = f[x.dtype], (N.POLICY_LOGITS if logits else N.POLICY_PROBS)
    d.value_type, d.returns_type = f[values.dtype], f[returns.dtype]
    d.action_type = N.PPO_ACT_U8 if actions.dtype == np.uint8 else N.PPO_ACT_I64
    assert old.dtype == np.float32
    rc = lib.sgw_ppo_loss(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == N.OK, lib.sgw_last_error()
    torch.cuda.synchronize()
    for g in (gd, gv, rows, terms, ws):
        assert g is None or g.intact(), "bytes outside an output were written"
    out = dict(terms=terms.numpy(), grad_dist=None, grad_values=gv.numpy() if gv else None, rows=rows.numpy().reshape(n, 3) if rows else None)
    if gd:
        flat_gd = gd.numpy()
        assert (flat_gd[:off].view(np.uint8) == 0xA5).all(), "the gradient wrote before its base"
        full = flat_gd[off:].reshape(n, stride)
        gaps = full[:, na:].copy().view(np.uint8)
        assert (gaps == 0xA5).all(), "the gradient wrote between the rows"
        out["grad_dist"] = full[:, :na].copy()
    return out


def same_nans(got, want):
    return np.array_equal(np.isnan(got), np.isnan(want))


def check(got, info, ctx, dist_dtype=np.float64, value_dtype=np.float64):
    """The call's outputs against the restatement, within the formulas (float32 gradients: the float64 value rounded once)."""
    tol = LC.tolerances(info, autograd=False)

    def within(g, w, t, what):
        assert same_nans(g, w), (ctx, what, "NaN pattern")
        with np.errstate(all="ignore"):
            err = np.abs(np.asarray(g, np.float64) - np.asarray(w, np.float64)) / np.maximum(t, 1e-300)
        share = float(np.nanmax(err)) if np.isfinite(err).any() else 0.0
        assert share <= 1.0, (ctx, what, share)

    want_terms = np.array([info["L"], info["Pm"], info["M"], info["Hm"]])
    within(got["terms"], want_terms, np.array([tol["L"], tol["Pm"], tol["M"], tol["Hm"]]), "terms")
    if got["rows"] is not None:
        within(got["rows"], np.stack([info["P"], info["d2"], info["H"]], axis=1), np.stack([tol["P"], tol["d2"], tol["H"]], axis=1), "row terms")
    if got["grad_dist"] is not None:
        want = LC.rounded(info["grad_dist"], dist_dtype)
        assert got["grad_dist"].dtype == np.dtype(dist_dtype)
        within(got["grad_dist"], want, tol["grad_dist"] + (LC.f32_slack(want) if dist_dtype == np.float32 else 0.0), "dL/ddist")
    if got["grad_values"] is not None:
        want = LC.rounded(info["grad_values"], value_dtype)
        assert got["grad_values"].dtype == np.dtype(value_dtype)
        within(got["grad_values"], want, tol["grad_values"] + (LC.f32_slack(want) if value_dtype == np.float32 else 0.0), "dL/dvalues")


def branches_are_clear(info):
    mar = LC.branch_margins(info, exact_ends=True)
    assert mar["ratio"] > LC.MARGIN and mar["surrogates"] > LC.MARGIN and mar["clamp_rows"].min() > LC.MARGIN, mar


# ------------------------------------------------------------------------------------------------------------- the reference's fixture
def fixture_arrays(s, bits):
    ft = np.float64 if bits == 64 else np.float32
    return s["probs"].astype(ft), s["values"].astype(ft), s["actions"], s["old_log_probs"], s["returns"].astype(ft)


@pytest.mark.parametrize("bits", (64, 32))
def test_fixture_through_the_abi(torch_cuda, bits):
    for tag, s in SETS.items():
        x, v, a, old, R = fixture_arrays(s, bits)
        info = LC.restate(x, False, v, a, old, R, s["eps_clip"], s["entropy_coef"])
        if bits == 32:
            branches_are_clear(info)                                   # (the casts moved nothing across a threshold)
        got = abi_loss(torch_cuda, x, v, a, old, R, s["eps_clip"], s["entropy_coef"])
        check(got, info, (tag, bits), x.dtype.type, v.dtype.type)
        if bits == 64:                                                 # ... and against the reference itself
            tol = LC.tolerances(info)
            assert abs(got["terms"][0] - s["loss"]) <= tol["L"]
            assert (np.abs(got["rows"][:, 2] - s["entropies"]) <= tol["H"]).all()
            assert (np.abs(got["grad_dist"] - s["grad_probs"]) <= tol["grad_dist"]).all()
            assert (np.abs(got["grad_values"] - s["grad_values"]) <= tol["grad_values"]).all()


@pytest.mark.parametrize("bits", (64, 32))
def test_fixture_through_the_python_entry_points(torch_cuda, bits):
    torch = torch_cuda
    from sorrel_amd import losses
    from sorrel_amd.models import ActionProbs

    for tag, s in SETS.items():
        x, v, a, old, R = fixture_arrays(s, bits)
        info = LC.restate(x, False, v, a, old, R, s["eps_clip"], s["entropy_coef"])
        tx, tv, ta, to, tr = (torch.from_numpy(t).to(DEV) for t in (x, v, a, old, R))
        res = losses.ppo_loss_terms(ActionProbs(tx), tv, ta, to, tr, s["eps_clip"], s["entropy_coef"], row_terms=True)
        got = dict(terms=res.terms.cpu().numpy(), rows=res.row_terms.cpu().numpy(), grad_dist=res.grad_dist.cpu().numpy(), grad_values=res.grad_values.cpu().numpy())
        check(got, info, (tag, bits, "terms"), x.dtype.type, v.dtype.type)
        assert res.loss.dim() == 0 and res.loss.item() == got["terms"][0] and res.entropy.item() == got["terms"][3]
        # a bare tensor counts as probabilities; out= hands back the same object
        assert losses.ppo_loss_terms(tx, tv, ta, to, tr, s["eps_clip"], s["entropy_coef"], out=res) is res
        # the autograd function: the same loss, and .grad = the saved gradients (times an incoming gradient of 1)
        px, pv = tx.clone().requires_grad_(True), tv.clone().requires_grad_(True)
        L = losses.ppo_loss(ActionProbs(px), pv, ta, to, tr, s["eps_clip"], s["entropy_coef"])
        assert L.dim() == 0 and L.dtype == torch.float64 and L.item() == got["terms"][0]
        L.backward()
        assert torch.equal(px.grad, res.grad_dist) and torch.equal(pv.grad, res.grad_values)


# ------------------------------------------------------------------------------------------------------------- a grid against the restatement
RATIOS = (0.0, 0.0, 2.0, -2.0, 0.5, 3.0, -0.5, -3.0)        # the ratios' distances from 1 in multiples of eps_clip (eps_clip 0: of 0.1, and 1 itself becomes 1.3)


def batch_of(rng, n, na, logits, dtype, eps_clip, c, vdtype, rdtype, adtype, zeros=True):
    """Rows, values, actions, returns and stored log-probabilities offset from the restatement's own so that the ratios fall on chosen
    sides of the clip range."""
    if logits:
        x = rng.integers(-32, 33, size=(n, na)).astype(np.float64) / 8.0
    else:
        x = rng.integers(1, 64, size=(n, na)).astype(np.float64)
        if zeros and na > 1:
            x[rng.random((n, na)) < 0.2] = 0.0
            x[np.arange(n), rng.integers(0, na, size=n)] += 3.0                                # (never an all-zero row)
        x /= 1024.0
    x = x.astype(dtype)
    v = (rng.integers(-40, 41, size=n) / 16.0).astype(vdtype)
    R = (rng.integers(-40, 41, size=n) / 16.0 + 1.0 / 32.0).astype(rdtype)                     # (never equal to v: A != 0)
    a = rng.integers(0, na, size=n).astype(adtype)
    now = LC.restate(x, logits, v, a, np.zeros(n, np.float32), R, eps_clip, c)["lp"]
    step = eps_clip if eps_clip > 0.0 else 0.1
    target = 1.0 + np.array([RATIOS[k % len(RATIOS)] for k in range(n)]) * step
    if eps_clip == 0.0:
        target[target == 1.0] = 1.3
    old = (now - np.log(target)).astype(np.float32)
    return x, v, a, old, R


@pytest.mark.parametrize("na", (1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 256))
def test_grid_against_the_restatement(torch_cuda, na):
    rng = np.random.default_rng(7000 + na)
    case = 0
    for n in (1, 63, 64, 65, 257):
        for logits in (False, True):
            # (dist type, wider stride, dist's base one element off, action / value / return types, the gradient's base one element off);
            # seven layouts against rules of period 2, 3, 5 and 11: every coefficient rule meets every layout
            for dtype, wider, misalign, adtype, vdtype, rdtype, grad_off in ((np.float32, False, False, np.int64, np.float32, np.float32, False),
                                                                             (np.float32, True, False, np.uint8, np.float64, np.float32, False),
                                                                             (np.float32, False, True, np.int64, np.float32, np.float64, False),
                                                                             (np.float64, False, False, np.uint8, np.float64, np.float64, False),
                                                                             (np.float64, True, False, np.int64, np.float32, np.float64, False),
                                                                             (np.float64, False, True, np.uint8, np.float32, np.float32, False),
                                                                             (np.float32, False, False, np.uint8, np.float64, np.float64, True)):
                case += 1
                eps_clip = 0.0 if case % 11 == 3 else (0.2 if case % 2 else 0.05)
                c = 0.0 if case % 5 == 1 else 0.01
                vc = (0.5, 0.25, 1.0)[case % 3]
                x, v, a, old, R = batch_of(rng, n, na, logits, dtype, eps_clip, c, vdtype, rdtype, adtype)
                info = LC.restate(x, logits, v, a, old, R, eps_clip, c, vc)
                assert not info["bad"].any()
                branches_are_clear(info)
                stride = na + (3 if wider else 0) if not (wider and na % 4 == 0) else na + 4   # (a wider stride that keeps 16-byte rows, too)
                got = abi_loss(torch_cuda, x, v, a, old, R, eps_clip, c, vc, logits=logits, stride=stride, misalign=misalign,
                               grad_off=grad_off)
                check(got, info, dict(na=na, n=n, logits=logits, dtype=dtype.__name__, stride=stride, misalign=misalign, eps=eps_clip, c=c, vc=vc,
                                      acts=adtype.__name__, grad_off=grad_off), dtype, vdtype)


def test_ties_of_the_two_surrogates(torch_cuda):
    """``s1 == s2``: the rows ``tests/test_ppo_loss_cpu.py`` checks on the restatement, through the ABI.  A ratio of exactly 1 (one
    action: ``lp = log(1 - 2^-52) = -2^-52``, which the float32 ``old`` holds) inside the one-point range of ``eps_clip`` 0, and ``A == 0``
    outside the range; the second batch has two actions so that a gradient does flow to the weights."""
    A = np.array([1.0, -1.0, 2.0, 0.0])
    ones = np.full((4, 1), 3.0)
    old = np.full(4, -2.0 ** -52, np.float32)
    info = LC.restate(ones, False, np.zeros(4), np.zeros(4, np.int64), old, A, 0.0, 0.0)
    assert (info["r"] == 1.0).all() and (info["s1"] == info["s2"]).all() and info["inside"].all() and np.array_equal(info["gr"], A)
    got = abi_loss(torch_cuda, ones, np.zeros(4), np.zeros(4, np.int64), old, A, 0.0, 0.0)
    check(got, info, "ties inside")
    assert np.array_equal(got["rows"][:, 0], -A) and (got["grad_dist"] == 0.0).all()
    two = np.tile(np.array([[0.25, 0.75]]), (4, 1))
    v = np.array([0.5, -1.0, 2.0, 0.0])
    old2 = np.array([0.5, -0.5, 1.0, -2.0], np.float32)                      # ratios far outside the range
    info = LC.restate(two, False, v, np.array([0, 1, 0, 1]), old2, v, 0.2, 0.01)
    assert (info["A"] == 0.0).all() and (info["s1"] == info["s2"]).all() and not info["inside"].any() and (info["gr"] == 0.0).all()
    got = abi_loss(torch_cuda, two, v, np.array([0, 1, 0, 1]), old2, v, 0.2, 0.01)
    check(got, info, "ties outside")
    assert (got["rows"][:, :2] == 0.0).all() and np.abs(got["grad_dist"]).max() > 0 and (got["grad_values"] == 0.0).all()


def test_more_row_tiles_than_workgroups_and_identical_bits(torch_cuda):
    n = LC.max_blocks() * 256 + 3
    assert n == 524291
    rng = np.random.default_rng(77)
    x, v, a, old, R = batch_of(rng, n, 2, False, np.float64, 0.2, 0.01, np.float64, np.float64, np.uint8)
    info = LC.restate(x, False, v, a, old, R, 0.2, 0.01)
    branches_are_clear(info)
    one = abi_loss(torch_cuda, x, v, a, old, R, 0.2, 0.01)
    check(one, info, "strided tiles")
    assert np.abs(one["grad_dist"][-260:]).max() > 0                       # (the rows of the last, strided-to tile are written)
    two = abi_loss(torch_cuda, x, v, a, old, R, 0.2, 0.01)
    for k in ("terms", "rows", "grad_dist", "grad_values"):
        assert np.array_equal(one[k].view(np.uint64), two[k].view(np.uint64)), k


# ------------------------------------------------------------------------------------------------------------- invalid rows, optional outputs
@pytest.mark.parametrize("na", (3, 8, 20))
def test_invalid_rows_are_nan_and_their_neighbours_are_untouched(torch_cuda, na):
    rng = np.random.default_rng(na)
    n = 70
    for logits in (False, True):
        x, v, a, old, R = batch_of(rng, n, na, logits, np.float64, 0.2, 0.01, np.float64, np.float64, np.int64, zeros=False)
        clean = LC.restate(x, logits, v, a, old, R, 0.2, 0.01)
        a = a.copy()
        a[3], a[64] = na, -1                                               # an action out of range, either side
        if logits:
            x[5, 1] = np.inf
            x[6, 0] = np.nan
            x[20] = -np.inf
        else:
            x[5, 1] = -0.25
            x[6, 0] = np.nan
            x[20] = 0.0
            x[40, na - 1] = np.inf
        info = LC.restate(x, logits, v, a, old, R, 0.2, 0.01)
        bad = info["bad"]
        assert bad.nonzero()[0].tolist() == ([3, 5, 6, 20, 64] if logits else [3, 5, 6, 20, 40, 64])
        got = abi_loss(torch_cuda, x, v, a, old, R, 0.2, 0.01, logits=logits)
        assert np.isnan(got["terms"]).all()                                # the means become NaN
        assert np.isnan(got["rows"][bad]).all() and np.isnan(got["grad_dist"][bad]).all() and np.isnan(got["grad_values"][bad]).all()
        tol = LC.tolerances(clean, autograd=False)
        good = ~bad
        assert np.isfinite(got["rows"][good]).all() and np.isfinite(got["grad_dist"][good]).all()
        assert (np.abs(got["grad_dist"][good] - clean["grad_dist"][good]) <= tol["grad_dist"][good]).all()
        assert (np.abs(got["rows"][good, 0] - clean["P"][good]) <= tol["P"][good]).all()
        assert (np.abs(got["grad_values"][good] - clean["grad_values"][good]) <= tol["grad_values"][good]).all()


def test_null_optional_outputs_and_no_rows(torch_cuda):
    rng = np.random.default_rng(12)
    for na in (4, 40):
        x, v, a, old, R = batch_of(rng, 300, na, False, np.float32, 0.2, 0.01, np.float32, np.float32, np.int64)
        info = LC.restate(x, False, v, a, old, R, 0.2, 0.01)
        branches_are_clear(info)
        for want_gd, want_gv, want_rows in ((False, False, False), (True, False, False), (False, True, True)):
            got = abi_loss(torch_cuda, x, v, a, old, R, 0.2, 0.01, want_gd=want_gd, want_gv=want_gv, want_rows=want_rows)
            check(got, info, (na, want_gd, want_gv, want_rows), np.float32, np.float32)
    # n == 0: nothing is launched, nothing is written
    torch = torch_cuda
    lib = N.load()
    terms = Guarded(torch, 4, np.float64)
    d = N.SgwPpoLossDesc()
    d.dist = d.values = d.actions = d.old_log_probs = d.returns = terms.ptr
    d.out_terms = terms.ptr
    d.n, d.row_stride, d.num_actions = 0, 4, 4
    d.eps_clip = 0.2
    assert lib.sgw_ppo_loss(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == N.OK
    torch.cuda.synchronize()
    assert terms.intact() and (terms.numpy().view(np.uint8) == 0xA5).all()


# ------------------------------------------------------------------------------------------------------------- autograd, capture
def test_backward_gives_the_gradients_of_ppo_loss_terms(torch_cuda):
    torch = torch_cuda
    from sorrel_amd import losses
    from sorrel_amd.models import ActionLogits

    rng = np.random.default_rng(21)
    count, E, na = 5, 67, 6
    x, v, a, old, R = batch_of(rng, count * E, na, True, np.float32, 0.2, 0.01, np.float32, np.float64, np.uint8)
    tx = torch.from_numpy(x).to(DEV).requires_grad_(True)
    tv = torch.from_numpy(v).to(DEV).view(count, E).requires_grad_(True)                     # a ring segment [count, E]
    ta, to, tr = (torch.from_numpy(t).to(DEV).view(count, E) for t in (a, old, R))
    res = losses.ppo_loss_terms(ActionLogits(tx.detach()), tv.detach(), ta, to, tr, 0.2, 0.01, 0.25)
    check(dict(terms=res.terms.cpu().numpy(), rows=None, grad_dist=res.grad_dist.cpu().numpy(), grad_values=res.grad_values.cpu().numpy().reshape(-1)),
          LC.restate(x, True, v, a, old, R, 0.2, 0.01, 0.25), "segment", np.float32, np.float32)
    L = losses.ppo_loss(ActionLogits(tx), tv, ta, to, tr, 0.2, 0.01, 0.25)
    assert torch.equal(L, res.loss)
    L.backward()
    assert tx.grad.shape == tx.shape and tv.grad.shape == (count, E)
    assert torch.equal(tx.grad, res.grad_dist) and torch.equal(tv.grad, res.grad_values)
    tx.grad = None
    (2.0 * losses.ppo_loss(ActionLogits(tx), tv, ta, to, tr, 0.2, 0.01, 0.25)).backward()    # an incoming gradient of 2: exact doubling
    assert torch.equal(tx.grad, 2.0 * res.grad_dist)
    with pytest.raises(ValueError):
        losses.ppo_loss_terms(tx.detach(), tv.detach().cpu(), ta, to, tr, 0.2, 0.01)
    cpu = [t.detach().cpu() for t in (tx, tv, ta, to, tr)]
    with pytest.raises(ValueError):                                                          # an out= that lives on another device
        losses.ppo_loss_terms(ActionLogits(tx.detach()), tv.detach(), ta, to, tr, 0.2, 0.01, out=losses.ppo_loss_terms(ActionLogits(cpu[0]), *cpu[1:], 0.2, 0.01))


def test_a_captured_call_replays_on_new_inputs(torch_cuda):
    torch = torch_cuda
    from sorrel_amd import losses
    from sorrel_amd.models import ActionProbs

    rng = np.random.default_rng(33)
    n, na = 3 * 256 + 11, 5
    x, v, a, old, R = batch_of(rng, n, na, False, np.float64, 0.2, 0.01, np.float64, np.float64, np.int64)
    tx, tv, ta, to, tr = (torch.from_numpy(t).to(DEV) for t in (x, v, a, old, R))
    res = losses.ppo_loss_terms(ActionProbs(tx), tv, ta, to, tr, 0.2, 0.01, row_terms=True)    # (code objects loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert losses.ppo_loss_terms(ActionProbs(tx), tv, ta, to, tr, 0.2, 0.01, out=res, row_terms=True) is res
    torch.cuda.synchronize()
    x2, v2, a2, old2, R2 = batch_of(rng, n, na, False, np.float64, 0.2, 0.01, np.float64, np.float64, np.int64)
    assert not np.array_equal(x, x2)
    for t, h in ((tx, x2), (tv, v2), (ta, a2), (to, old2), (tr, R2)):
        t.copy_(torch.from_numpy(h))
    res.terms.fill_(-1.0)
    res.grad_dist.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    info = LC.restate(x2, False, v2, a2, old2, R2, 0.2, 0.01)
    branches_are_clear(info)
    check(dict(terms=res.terms.cpu().numpy(), rows=res.row_terms.cpu().numpy(), grad_dist=res.grad_dist.cpu().numpy(), grad_values=res.grad_values.cpu().numpy()),
          info, "replay")
    eager = losses.ppo_loss_terms(ActionProbs(tx), tv, ta, to, tr, 0.2, 0.01, row_terms=True)
    torch.cuda.synchronize()
    assert eager.terms.data_ptr() != res.terms.data_ptr()
    assert torch.equal(eager.terms, res.terms) and torch.equal(eager.grad_dist, res.grad_dist) and torch.equal(eager.grad_values, res.grad_values)


# ------------------------------------------------------------------------------------------------------------- end to end
E2E_FLOOR = 2.0 ** -48        # of the largest reference gradient: see the test's docstring


def test_one_learner_step_against_the_references_parameter_gradients(torch_cuda):
    """A four-layer tanh actor and critic with the reference's initial weights, on the fixture's states, one backward: (a) through
    ``ppo_loss`` and (b) through ``_ppo_loss_torch``, both on the device.  (b) is torch's own arithmetic, not code under test: its
    distance from the reference's parameter gradients (computed on a CPU) measures what the device's GEMMs and tanh alone change.  (a)
    must lie within twice that distance plus a floor of 2^-48 of the largest reference gradient -- 32 float64 roundings: a parameter's
    gradient is a sum over 64 rows, taken in another order, of products that passed four layers.  The test asserts that (b) stays
    within a quarter of the floor; the smallest power of two for which the measured distance does is 2^-49, and one more bit is left
    for another GEMM path of the library.
    Measured on the MI355X: see DESIGN.md 0.15."""
    torch = torch_cuda
    from sorrel_amd import losses
    from sorrel_amd.models import ActionProbs

    assert E2E is not None
    s = SETS[E2E["tag"]]
    nin, hid, na = int(E2E["inputs"]), int(E2E["hidden"]), s["na"]
    nn = torch.nn

    def build():
        actor = nn.Sequential(nn.Linear(nin, hid), nn.Tanh(), nn.Linear(hid, 2 * hid), nn.Tanh(), nn.Identity(), nn.Linear(2 * hid, hid), nn.Tanh(),
                              nn.Linear(hid, na), nn.Softmax(dim=-1))
        critic = nn.Sequential(nn.Linear(nin, hid), nn.Tanh(), nn.Linear(hid, 2 * hid), nn.Tanh(), nn.Identity(), nn.Linear(2 * hid, hid), nn.Tanh(),
                               nn.Linear(hid, 1))
        net = nn.ModuleDict(dict(actor=actor, critic=critic)).double()
        net.load_state_dict({name: torch.from_numpy(E2E["w:" + name]) for name in E2E["names"]})
        return net.to(DEV)

    states = torch.from_numpy(E2E["states"]).to(DEV)
    ta, to, tr = (torch.from_numpy(s[k]).to(DEV) for k in ("actions", "old_log_probs", "returns"))
    scale = max(float(np.abs(E2E["g:" + name]).max()) for name in E2E["names"])
    dist = {}
    for which in ("kernel", "torch"):
        net = build()
        probs, values = net["actor"](states), net["critic"](states).squeeze(-1)
        if which == "kernel":
            L = losses.ppo_loss(ActionProbs(probs), values, ta, to, tr, s["eps_clip"], s["entropy_coef"])
        else:
            L = losses._ppo_loss_torch(probs, False, values, ta, to, tr, s["eps_clip"], s["entropy_coef"])[0]
        L.backward()
        grads = dict(net.named_parameters())
        dist[which] = max(float(np.abs(grads[name].grad.cpu().numpy() - E2E["g:" + name]).max()) for name in E2E["names"])
    floor = E2E_FLOOR * scale
    print(f"end to end: ppo_loss {dist['kernel']:.3e}, _ppo_loss_torch {dist['torch']:.3e} from the reference's parameter gradients; floor {floor:.3e} "
          f"(largest gradient {scale:.3e})")
    assert dist["torch"] <= floor / 4
    assert dist["kernel"] <= 2 * dist["torch"] + floor
