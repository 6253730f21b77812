"""``sgw_iqn_loss`` on the device: the reference's fixture (``tests/golden/iqn_loss``) through the C ABI and through both Python entry
points; a pruned product of quantile counts (every lane-group bucket full and one past), batch sizes around the rows of a wave and of a
tile, and action counts, with both action types and both ``valid`` types (weights other than 0 / 1 included) -- all against the NumPy
restatement (``tests/iqn_loss_common.py``, itself pinned by the fixture in ``tests/test_iqn_loss_cpu.py``) BIT FOR BIT; bases one element
off the 16-byte boundary and each optional output NULL in turn; invalid rows and the bytes around every output and the workspace; more
row tiles than workgroups, twice, with identical bits; ``iqn_loss(...).backward()`` at a leaf and through a ``Linear`` head; a replayed
capture; and a batch straight from ``TurnBuffer.sample``.

Bounds.  There is no libm in this loss, so the kernel against the restatement has no tolerance at all; the reference's autograd and
``mean()`` may order sums differently, and those comparisons use the FORMULAS of ``tests/iqn_loss_common.py``.  No expectation comes
from the kernel."""
import ctypes as C

import numpy as np
import pytest

from sorrel_amd import _native as N
from tests import iqn_loss_common as LC
from tests.gpu_common import torch_cuda  # noqa: F401
from tests.learner_common import DEV, Guarded

pytestmark = pytest.mark.gpu

SETS = LC.load_fixture()
INPUTS = ("q_expected", "taus", "q_next_local", "q_next_target", "actions", "rewards", "dones", "valid")
OUTPUTS = ("grad", "next_actions", "row_terms", "td_error")


def abi_loss(torch, qe, taus, ql, qt, actions, rewards, dones, valid, discount, *, off=(), skip=()):
    """One ``sgw_iqn_loss`` call over host arrays; the inputs named in ``off`` and the outputs named in ``off`` start one element past
    a 16-byte boundary; the outputs named in ``skip`` are NULL.  Every output and the workspace sit inside guards, which must come back
    untouched.  Returns a dict of host arrays (None for a skipped output)."""
    lib = N.load()
    B, Nq, A = qe.shape
    keep = {}
    for name, a in zip(INPUTS, (qe, taus, ql, qt, actions, rewards, dones, valid)):
        a = np.ascontiguousarray(a).ravel()
        flat = torch.from_numpy(np.concatenate([np.zeros(1, a.dtype), a])).to(DEV)
        keep[name] = flat[1:] if name in off else flat[1:].clone()
        assert name not in off or keep[name].data_ptr() % 16 == a.dtype.itemsize % 16
    sizes = dict(grad=(B * Nq * A, np.float32), next_actions=(B, np.int64), row_terms=(B, np.float64), td_error=(B * Nq * Nq, np.float32))
    outs = {k: (None if k in skip else Guarded(torch, n, dt, shift=np.dtype(dt).itemsize if k in off else 0)) for k, (n, dt) in sizes.items()}
    terms = Guarded(torch, 1, np.float64)
    need = int(lib.sgw_iqn_loss_workspace_bytes(B, Nq))
    assert need == LC.blocks_of(B, Nq) * 8
    ws = Guarded(torch, need // 8, np.float64)
    d = N.SgwIqnLossDesc()
    d.q_expected, d.taus, d.q_next_local, d.q_next_target = (keep[k].data_ptr() for k in INPUTS[:4])
    d.actions, d.rewards, d.dones, d.valid = (keep[k].data_ptr() for k in INPUTS[4:])
    d.out_grad_expected, d.out_next_actions, d.out_row_terms, d.out_td_error = (outs[k].ptr if outs[k] else None for k in OUTPUTS)
    d.out_terms, d.workspace, d.workspace_bytes = terms.ptr, ws.ptr, need
    d.n, d.num_quantiles, d.num_actions, d.discount = B, Nq, A, discount
    d.action_type = N.PPO_ACT_U8 if np.asarray(actions).dtype == np.uint8 else N.PPO_ACT_I64
    d.valid_type = N.POLICY_F64 if np.asarray(valid).dtype == np.float64 else N.POLICY_F32
    rc = lib.sgw_iqn_loss(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == N.OK, lib.sgw_last_error()
    torch.cuda.synchronize()
    for g in list(outs.values()) + [terms, ws]:
        assert g is None or g.intact(), "bytes outside an output were written"
    shapes = dict(grad=(B, Nq, A), next_actions=(B,), row_terms=(B,), td_error=(B, Nq, Nq))
    got = {k: (outs[k].numpy().reshape(shapes[k]) if outs[k] else None) for k in OUTPUTS}
    got["L"] = terms.numpy()
    return got


def check(got, info, ctx):
    """Every output against the restatement, bit for bit."""
    for key, want in (("grad", info["grad"]), ("next_actions", info["next_actions"]), ("row_terms", info["row_terms"]), ("td_error", info["td_error"])):
        if got.get(key) is not None:
            LC.same_bits(got[key], want, key, ctx)
    LC.same_bits(got["L"], np.array([info["L"]], np.float64), "L", ctx)


def of_result(res):
    return dict(grad=res.grad_expected.cpu().numpy(), next_actions=res.next_actions.cpu().numpy(),
                row_terms=None if res.row_terms is None else res.row_terms.cpu().numpy(),
                td_error=None if res.td_error is None else res.td_error.cpu().numpy(), L=res.terms.cpu().numpy())


def at_action(grad, actions):
    B = grad.shape[0]
    return grad[np.arange(B), :, np.asarray(actions).reshape(B).astype(np.int64)]


def against_the_reference(got, s, info, ctx):
    LC.same_bits(got["next_actions"], info["next_actions"], "next_actions", ctx)
    LC.same_bits(got["td_error"], s["td_error"], "td_error against the reference", ctx)
    B = s["B"]
    mask = np.ones(s["grad_expected"].shape, bool)
    mask[np.arange(B), :, s["actions"].reshape(B)] = False
    LC.same_bits(got["grad"][mask], s["grad_expected"][mask], "the gradient's zeros against the reference", ctx)
    tol = LC.tolerances(info)
    err = np.abs(at_action(got["grad"], s["actions"]).astype(np.float64) - at_action(s["grad_expected"], s["actions"]).astype(np.float64))
    share = float(np.max(err / np.maximum(tol["grad"], 1e-300)))
    loss_share = abs(float(got["L"][0]) - float(s["loss"])) / max(tol["L"], 1e-300)
    print(f"{ctx}: gradient {share:.4f}, loss {loss_share:.4f} of the tolerance against the reference")
    assert share <= 1.0 and loss_share <= 1.0, (ctx, share, loss_share)


# ------------------------------------------------------------------------------------------------------------- the fixture
def test_fixture_through_the_abi(torch_cuda):
    for tag, s in sorted(SETS.items()):
        info = LC.restate(*LC.inputs_of(s))
        got = abi_loss(torch_cuda, *LC.inputs_of(s))
        check(got, info, tag)
        against_the_reference(got, s, info, tag)


def test_fixture_through_the_python_entry_points(torch_cuda):
    torch = torch_cuda
    from sorrel_amd import losses

    for tag, s in sorted(SETS.items()):
        info = LC.restate(*LC.inputs_of(s))
        args = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in LC.inputs_of(s)[:8]) + (s["discount"],)
        res = losses.iqn_loss_terms(*args, row_terms=True, td_error=True)
        assert res.loss.dtype == torch.float64 and res.loss.dim() == 0 and res.grad_expected.dtype == torch.float32
        got = of_result(res)
        check(got, info, tag)
        against_the_reference(got, s, info, tag)
        L = losses.iqn_loss(*args)
        assert L.dtype == torch.float64 and L.dim() == 0 and not L.requires_grad
        LC.same_bits(L.cpu().numpy().reshape(1), np.array([info["L"]]), "iqn_loss", tag)


# ------------------------------------------------------------------------------------------------------------- shapes
# every value of each axis meets small and large values of the other two: (B, A) pairs per quantile count
SWEEP = {
    1: ((1, 1), (257, 256), (64, 5), (5, 64)),
    2: ((3, 2), (257, 17), (63, 256), (4, 1)),
    3: ((4, 4), (65, 65), (1, 256), (257, 2)),
    8: ((5, 5), (64, 16), (3, 65), (257, 4)),
    9: ((63, 1), (1, 17), (65, 256), (4, 64)),
    12: ((64, 4), (3, 16), (257, 5), (5, 256), (1, 2)),
    16: ((65, 2), (4, 65), (1, 64), (63, 17)),
    17: ((257, 1), (3, 4), (5, 16), (64, 256)),
    32: ((1, 5), (63, 64), (4, 256), (65, 4)),
    33: ((3, 1), (64, 17), (5, 2), (257, 16), (4, 256)),
    64: ((4, 2), (1, 65), (63, 4), (65, 16), (3, 256), (64, 1), (5, 17), (257, 5)),
}


def test_the_sweep_covers_every_axis():
    assert set(SWEEP) == {1, 2, 3, 8, 9, 12, 16, 17, 32, 33, 64}
    assert {b for v in SWEEP.values() for b, _ in v} == {1, 3, 4, 5, 63, 64, 65, 257}
    assert {a for v in SWEEP.values() for _, a in v} == {1, 2, 4, 5, 16, 17, 64, 65, 256}


@pytest.mark.parametrize("Nq", sorted(SWEEP))
def test_sweep_against_the_restatement(torch_cuda, Nq):
    rng = np.random.default_rng(100 + Nq)
    for k, (B, A) in enumerate(SWEEP[Nq]):
        adt = np.uint8 if (k + Nq) % 2 else np.int64
        vdt = np.float32 if (k // 2 + Nq) % 2 else np.float64
        case = LC.random_case(rng, B, Nq, A, action_dtype=adt, valid_dtype=vdt, weights=k % 2 == 0)
        info = LC.restate(*case, 0.970299)
        mag = np.abs(info["td_error"])
        assert B * Nq < 30 or ((mag <= 1).any() and (mag > 1).any())
        check(abi_loss(torch_cuda, *case, 0.970299), info, f"N={Nq} B={B} A={A} {np.dtype(adt).name} {np.dtype(vdt).name}")


def test_misaligned_bases_and_null_outputs(torch_cuda):
    rng = np.random.default_rng(5)
    for B, Nq, A in ((37, 12, 4), (5, 3, 8)):                       # A a multiple of 4: the 16-byte stores must step aside for the gradient's base
        case = LC.random_case(rng, B, Nq, A, valid_dtype=np.float32)
        info = LC.restate(*case, 0.9)
        for name in INPUTS + ("grad", "td_error"):
            check(abi_loss(torch_cuda, *case, 0.9, off=(name,)), info, f"{name} one element off")
        check(abi_loss(torch_cuda, *case, 0.9, off=INPUTS + ("grad", "td_error")), info, "everything one element off")
        for name in OUTPUTS:
            got = abi_loss(torch_cuda, *case, 0.9, skip=(name,))
            assert got[name] is None
            check(got, info, f"{name} is NULL")
        check(abi_loss(torch_cuda, *case, 0.9, skip=OUTPUTS), info, "every optional output is NULL")


def test_ties_and_nans_in_the_action_choice(torch_cuda):
    rng = np.random.default_rng(8)
    B, Nq, A = 9, 5, 70                                             # more actions than lanes in a group: a lane's own scan and the merge
    case = list(LC.random_case(rng, B, Nq, A))
    ql = case[2]
    ql[0, :, :] = 0.25                                              # all tied: the first
    ql[1, :, :] = 0.25
    ql[1, :, 69] = 0.5
    ql[1, :, 9] = 0.5                                               # a tie across lanes
    ql[2, 1, 66] = np.nan
    ql[2, 3, 13] = np.nan                                           # the first NaN, in a later round of an earlier lane ... and
    ql[3, 0, 5] = np.nan
    ql[3, 0, 8] = np.inf                                            # a NaN beats +inf
    ql[4, :, :] = -np.inf
    ql[5, :, :] = np.nan
    ql[6, :, 3] = 0.0
    ql[6, :, 2] = -0.0
    ql[6, :, :2] = -1.0
    ql[6, :, 4:] = -1.0                                             # -0 == +0: the first
    info = LC.restate(*case, 0.9)
    assert info["next_actions"].tolist()[:7] == [0, 9, 13, 5, 0, 0, 2]
    check(abi_loss(torch_cuda, *case, 0.9), info, "ties and NaNs")


# ------------------------------------------------------------------------------------------------------------- invalid rows
@pytest.mark.parametrize("shape", ((6, 3, 5), (70, 12, 4), (5, 64, 17)))
def test_invalid_rows_are_nan_and_their_neighbours_are_untouched(torch_cuda, shape):
    rng = np.random.default_rng(17)
    B, Nq, A = shape
    case = list(LC.random_case(rng, B, Nq, A))
    clean = LC.restate(*case, 0.9)
    case[4][1, 0] = A                                               # one past the end
    case[4][B - 2, 0] = -1                                          # negative
    info = LC.restate(*case, 0.9)
    assert info["bad"].sum() == 2
    got = abi_loss(torch_cuda, *case, 0.9)
    check(got, info, f"invalid rows {shape}")
    for b in (1, B - 2):
        assert np.isnan(got["grad"][b]).all() and np.isnan(got["row_terms"][b]) and np.isnan(got["td_error"][b]).all()
    assert np.isnan(got["L"][0])
    good = np.ones(B, bool)
    good[[1, B - 2]] = False
    LC.same_bits(got["grad"][good], clean["grad"][good], "the neighbours' gradient")
    LC.same_bits(got["row_terms"][good], clean["row_terms"][good], "the neighbours' row terms")
    LC.same_bits(got["next_actions"], clean["next_actions"], "a* of every row")
    if A <= 255:
        u8 = list(case)
        u8[4] = np.where(case[4] < 0, 255, case[4]).astype(np.uint8)                 # uint8: 255 is out of range too
        check(abi_loss(torch_cuda, *u8, 0.9), info, f"invalid uint8 rows {shape}")


# ------------------------------------------------------------------------------------------------------------- reproducibility
def test_more_row_tiles_than_workgroups_and_identical_bits(torch_cuda):
    rng = np.random.default_rng(3)
    B, Nq, A = 524291, 2, 2
    assert -(-B // (LC.BLOCK // LC.group(Nq))) > 2 * LC.max_blocks()
    case = LC.random_case(rng, B, Nq, A, valid_dtype=np.float32)
    info = LC.restate(*case, 0.970299)
    first = abi_loss(torch_cuda, *case, 0.970299)
    second = abi_loss(torch_cuda, *case, 0.970299)
    check(first, info, "524291 rows")
    for key in OUTPUTS + ("L",):
        assert np.array_equal(LC.bits(first[key]), LC.bits(second[key])), key


# ------------------------------------------------------------------------------------------------------------- autograd
def device_case(torch, rng, B, Nq, A, **kw):
    case = LC.random_case(rng, B, Nq, A, **kw)
    return case, tuple(torch.from_numpy(x).to(DEV) for x in case)


def test_backward_gives_a_leaf_exactly_grad_expected(torch_cuda):
    torch = torch_cuda
    from sorrel_amd import losses

    rng = np.random.default_rng(21)
    case, dev = device_case(torch, rng, 65, 12, 5)
    info = LC.restate(*case, 0.970299)
    leaf = dev[0].clone().requires_grad_(True)
    other = dev[2].clone().requires_grad_(True)
    L = losses.iqn_loss(leaf, dev[1], other, *dev[3:], 0.970299)
    assert L.requires_grad and L.dtype == torch.float64 and L.dim() == 0
    L.backward()
    assert other.grad is None
    LC.same_bits(leaf.grad.cpu().numpy(), info["grad"], "the leaf's gradient")
    LC.same_bits(L.detach().cpu().numpy().reshape(1), np.array([info["L"]]), "L")
    terms = losses.iqn_loss_terms(*dev, 0.970299)
    assert torch.equal(terms.grad_expected, leaf.grad)
    cpu = tuple(t.cpu() for t in dev)
    with pytest.raises(ValueError, match="out="):
        losses.iqn_loss_terms(*dev, 0.970299, out=losses.iqn_loss_terms(*cpu, 0.970299))


def test_parameter_gradients_of_a_linear_head(torch_cuda):
    """A ``Linear(K, N A)`` head on ``[B, K]`` features, reshaped to ``[B, N, A]``; its parameter gradients through ``iqn_loss`` against
    ``_iqn_loss_torch`` on the same device tensors.  Both backward passes hand the head a float32 ``[B, N A]`` gradient ``g`` and let
    the same GEMM form ``dW = g^T x`` and ``db = sum_b g``.  The two ``g`` differ by at most ``t_bi`` = the gradient formula of
    ``tests/iqn_loss_common.py`` at the action taken (and are both exact zeros elsewhere), so

        |dW_(i a),k - dW'_(i a),k| <= sum_b t_bi |x_bk|  +  2 B 2^-24 sum_b |g_bia| |x_bk|

    the second term being two float32 GEMMs of B terms each, in whatever order (``B N`` terms per output element counts the N - 1
    structural zeros of a column; B bounds what is added).  ``db`` is the same with ``x = 1``.  Every quantity on the right comes from
    the restatement and the inputs."""
    torch = torch_cuda
    from sorrel_amd import losses

    rng = np.random.default_rng(44)
    B, Nq, A, K = 64, 12, 4, 10
    case, dev = device_case(torch, rng, B, Nq, A)
    torch.manual_seed(5)
    head = torch.nn.Linear(K, Nq * A).to(DEV)
    x = torch.from_numpy(rng.normal(size=(B, K)).astype(np.float32)).to(DEV)
    grads = []
    for fn in (losses.iqn_loss, lambda *a: losses._iqn_loss_torch(*a)[0]):
        head.zero_grad()
        qe = head(x).reshape(B, Nq, A)
        fn(qe, *dev[1:], 0.970299).backward()
        grads.append((head.weight.grad.cpu().numpy().astype(np.float64), head.bias.grad.cpu().numpy().astype(np.float64), qe.detach().cpu().numpy()))
    info = LC.restate(grads[0][2], *case[1:], 0.970299)
    mag = np.abs(info["td_error"].astype(np.float64))
    assert (np.abs(mag - 1.0) > 2.0 ** -20).all()                   # both paths take the same Huber branches
    act = case[4].reshape(B)
    t = np.zeros((B, Nq, A))
    t[np.arange(B), :, act] = LC.tolerances(info)["grad"]
    gabs = np.abs(info["grad"].astype(np.float64))
    xa = np.abs(x.cpu().numpy().astype(np.float64))
    bound_w = np.einsum("bq,bk->qk", t.reshape(B, -1), xa) + 2 * B * 2.0 ** -24 * np.einsum("bq,bk->qk", gabs.reshape(B, -1), xa)
    bound_b = t.reshape(B, -1).sum(axis=0) + 2 * B * 2.0 ** -24 * gabs.reshape(B, -1).sum(axis=0)
    (w0, b0, _), (w1, b1, _) = grads
    assert np.abs(w1).max() > 1e-5 and np.abs(b1).max() > 1e-5
    live = bound_w > 0
    assert np.array_equal(w0[~live], w1[~live]) and np.array_equal(b0[bound_b == 0], b1[bound_b == 0])
    share_w = float(np.max(np.abs(w0 - w1)[live] / bound_w[live]))
    share_b = float(np.max(np.abs(b0 - b1)[bound_b > 0] / bound_b[bound_b > 0]))
    print(f"Linear head: weight gradients {share_w:.4f}, bias gradients {share_b:.4f} of the bound")
    assert share_w <= 1.0 and share_b <= 1.0, (share_w, share_b)


# ------------------------------------------------------------------------------------------------------------- capture
def test_a_captured_call_replays_on_new_inputs(torch_cuda):
    torch = torch_cuda
    from sorrel_amd import losses

    rng = np.random.default_rng(33)
    B, Nq, A = 3 * 16 + 5, 12, 5
    case, dev = device_case(torch, rng, B, Nq, A)
    res = losses.iqn_loss_terms(*dev, 0.970299, row_terms=True, td_error=True)      # (code objects loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert losses.iqn_loss_terms(*dev, 0.970299, out=res, row_terms=True, td_error=True) is res
    torch.cuda.synchronize()
    case2 = LC.random_case(rng, B, Nq, A)
    assert not np.array_equal(case[0], case2[0])
    for t, h in zip(dev, case2):
        t.copy_(torch.from_numpy(h))
    res.terms.fill_(-1.0)
    res.grad_expected.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    check(of_result(res), LC.restate(*case2, 0.970299), "replay")
    eager = losses.iqn_loss_terms(*dev, 0.970299)
    torch.cuda.synchronize()
    assert eager.terms.data_ptr() != res.terms.data_ptr()
    assert torch.equal(eager.terms, res.terms) and torch.equal(eager.grad_expected, res.grad_expected)


# ------------------------------------------------------------------------------------------------------------- end to end
def test_a_sampled_batch_goes_straight_in(torch_cuda):
    torch = torch_cuda
    from sorrel_amd import losses
    from sorrel_amd.buffers import TurnBuffer

    rng = np.random.default_rng(9)
    cap, E, A_agents, n_act, Nq, B, n_frames = 16, 3, 2, 4, 8, 21, 2
    ring = TurnBuffer(cap, E, (A_agents, 1, 3, 3), device=DEV)
    ring.obs.copy_(torch.from_numpy(rng.normal(size=tuple(ring.obs.shape)).astype(np.float32)))
    ring.actions.copy_(torch.from_numpy(rng.integers(0, n_act, size=tuple(ring.actions.shape)).astype(np.uint8)))
    ring.rewards.copy_(torch.from_numpy((rng.integers(-3, 4, size=tuple(ring.rewards.shape)) * 0.5).astype(np.float32)))
    ring.dones.copy_(torch.from_numpy((rng.random(size=tuple(ring.dones.shape)) < 0.3).astype(np.float32)))
    ring.idx, ring.size = 0, cap
    torch.manual_seed(2)
    states, actions, rewards, next_states, dones, valid = ring.sample(B, agent=1, n_frames=n_frames)
    assert actions.shape == (B, 1) and valid.shape == (B, 1) and states.shape[0] == B
    assert set(np.unique(valid.cpu().numpy())) == {0.0, 1.0}
    head = torch.nn.Linear(states.shape[1], Nq * n_act).to(DEV)
    with torch.no_grad():
        qe, ql, qt = (head(s).reshape(B, Nq, n_act).contiguous() * k for s, k in ((states, 1.0), (next_states, 1.0), (next_states, 0.5)))
    taus = torch.rand((B, Nq, 1), device=DEV)
    res = losses.iqn_loss_terms(qe, taus, ql, qt, actions, rewards, dones, valid, 0.99 ** 3, row_terms=True, td_error=True)
    host = tuple(t.cpu().numpy() for t in (qe, taus, ql, qt, actions, rewards, dones, valid))
    info = LC.restate(*host, 0.99 ** 3)
    check(of_result(res), info, "a sampled batch")
    assert not info["bad"].any() and info["L"] > 0 and (info["row_terms"][valid.cpu().numpy().reshape(B) == 0] == 0).all()
