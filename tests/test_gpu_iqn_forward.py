"""``sgw_iqn_forward`` on the device: the reference's fixture (``tests/golden/iqn_forward``) through the C ABI and through ``IQN.quantiles`` /
``get_qvalues`` -- within ``2 E`` of the reference (``tests/iqn_forward_common.py``: a formula), the greedy actions equal, and EVERY kernel
output bit for bit against the NumPy restatement fed the kernel's own ``out_cos`` and taus --; a pruned product of shapes around the tile
sizes with float32 and uint8 states; strides, bases one element off a 16-byte boundary, each optional output NULL in turn, guard bytes
around every output and the workspace; 65 537 rows twice with identical bits and single rows of it alone; a NaN that stays in its row; the
keyed taus against a NumPy Philox; training mode's effective weights; a recorded graph replayed after states and weights changed; and a
Treasurehunt policy turn with ``IQNActor``, eager against ``capture_turn()``.  ``cosf`` is measured, not restated: ``COS_ULPS`` below."""
import ctypes as C

import numpy as np
import pytest

from sorrel_amd import _native as N
from tests import iqn_forward_common as FC
from tests.gpu_common import torch_cuda  # noqa: F401
from tests.learner_common import DEV, Guarded

pytestmark = pytest.mark.gpu

SETS = FC.load_fixture()
OUTPUTS = ("qvalues", "quantiles", "taus", "cos")
# the device library's cosf against float64 cos of the same float32 argument over [0, 64 pi): tools/bench_iqn_forward.py measured at most
# 1.1852 x 2^-24 over 2^20 taus x 64 frequencies (profiles/iqn_forward.txt); twice that, rounded up to a whole unit of 2^-24
COS_ULPS = 3


def abi_forward(torch, w, states, Nq, *, taus=None, key=None, idx=None, off=(), skip=(), stride=None, untouched=False):
    """One ``sgw_iqn_forward`` call over host arrays.  The weights and outputs named in ``off`` start one element past a 16-byte boundary;
    the outputs named in ``skip`` are NULL; ``stride``: the states' row stride in elements.  Every output and the workspace sit inside
    guards, which must come back untouched.  Returns a dict of host arrays (None for a skipped output)."""
    lib = N.load()
    states = np.ascontiguousarray(states)
    B, D = states.shape
    L, A = np.asarray(w["w_ff"]).shape[0], np.asarray(w["w_adv"]).shape[0]
    stride = D if stride is None else stride
    padded = np.zeros((B, stride), states.dtype)
    padded[:, :D] = states
    padded[:, D:] = 77                                                           # (what lies between rows is not read)
    keep = {"states": torch.from_numpy(padded if B else np.zeros((1, stride), states.dtype)).to(DEV)}     # (no rows: still a pointer)
    for name in FC.WEIGHTS:
        a = np.ascontiguousarray(w[name], np.float32).ravel()
        flat = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), a])).to(DEV)
        keep[name] = flat[1:] if name in off else flat[1:].clone()
        assert name not in off or keep[name].data_ptr() % 16 == 4
    sizes = dict(qvalues=B * A, quantiles=B * Nq * A, taus=B * Nq, cos=B * Nq * FC.N_COS)
    outs = {k: (None if k in skip else Guarded(torch, n, np.float32, shift=4 if k in off else 0)) for k, n in sizes.items()}
    need = int(lib.sgw_iqn_forward_workspace_bytes(B, L))
    assert need == B * L * 4
    ws = Guarded(torch, need // 4, np.float32, shift=4 if "workspace" in off else 0)
    d = N.SgwIqnForwardDesc()
    d.states = keep["states"].data_ptr()
    for name in FC.WEIGHTS:
        setattr(d, name, keep[name].data_ptr())
    d.out_qvalues, d.out_quantiles, d.out_taus, d.out_cos = (outs[k].ptr if outs[k] else None for k in OUTPUTS)
    d.workspace, d.workspace_bytes = ws.ptr, need
    d.n, d.state_stride = B, stride
    d.in_features, d.layer_size, d.num_quantiles, d.num_actions, d.n_cos = D, L, Nq, A, FC.N_COS
    d.state_type = 1 if states.dtype == np.uint8 else 0
    if taus is not None:
        keep["taus"] = torch.from_numpy(np.ascontiguousarray(taus, np.float32).reshape(B, Nq) if B else np.zeros((1, Nq), np.float32)).to(DEV)
        d.taus = keep["taus"].data_ptr()
    else:
        key = dict(key or {})
        d.seed, d.first_env, d.epoch, d.turn = key.get("seed", 3), key.get("first_env", 0), key.get("epoch", 0), key.get("turn", 1)
        d.num_envs, d.agent0 = key.get("num_envs", max(B, 1)), key.get("agent0", 0)
        if idx is not None:
            keep["idx"] = torch.from_numpy(np.ascontiguousarray(idx, np.int64)).to(DEV)
            d.idx = keep["idx"].data_ptr()
    rc = lib.sgw_iqn_forward(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == N.OK, lib.sgw_last_error()
    torch.cuda.synchronize()
    for g in list(outs.values()) + [ws]:
        assert g is None or g.intact(), "bytes outside an output were written"
    if untouched:
        assert all(g is None or (g.numpy().view(np.uint8) == 0xA5).all() for g in list(outs.values()) + [ws])
    shapes = dict(qvalues=(B, A), quantiles=(B, Nq, A), taus=(B, Nq), cos=(B, Nq, FC.N_COS))
    return {k: (outs[k].numpy().reshape(shapes[k]) if outs[k] else None) for k in OUTPUTS}


def check_bits(got, w, states, ctx, taus=None):
    """Everything behind the library's cosf, bit for bit: the restatement is fed the kernel's own cos; the cosines themselves lie within
    ``COS_ULPS`` units of float64 cos of the float32 argument that the kernel's own taus give."""
    quant, qv = FC.restate(w, states, got["cos"])
    FC.same_bits(got["quantiles"], quant, "quantiles", ctx)
    FC.same_bits(got["qvalues"], qv, "qvalues", ctx)
    if taus is not None:
        FC.same_bits(got["taus"], np.asarray(taus, np.float32).reshape(got["taus"].shape), "taus", ctx)
    args = FC.cos_args(got["taus"]).astype(np.float64)
    err = np.abs(got["cos"].astype(np.float64) - np.cos(args)) / FC.U
    print(f"{ctx}: cosf within {np.nanmax(err) if err.size else 0:.3f} x 2^-24 of float64 cos")
    assert not (err > COS_ULPS).any(), (ctx, float(np.nanmax(err)))


def to_net(torch, s, mode="eval"):
    from sorrel_amd.models import iqn as M

    net = M.IQN((s["D"],), s["A"], s["L"], seed=0, n_quantiles=s["N"], n_frames=1)
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in s["sd"].items()})
    net.train(mode == "train")
    return net.to(DEV)


# ------------------------------------------------------------------------------------------------------------- 1: the fixture
@pytest.mark.parametrize("tag", sorted(SETS))
def test_fixture_through_the_abi_and_the_module(torch_cuda, tag):
    torch = torch_cuda
    s = SETS[tag]
    for mode in ("eval", "u8", "train"):
        r = s[mode]
        x = s["states_u8"] if mode == "u8" else s["states"]
        ctx = f"{tag} {mode}"
        got = abi_forward(torch, r["w"], x, s["N"], taus=r["taus"])
        check_bits(got, r["w"], x, ctx, taus=r["taus"])
        q64, qv64, eq, eqv = FC.bound(r["w"], x, r["cos"], cos_other=got["cos"])
        share = max(float((np.abs(got["quantiles"].astype(np.float64) - r["quantiles"]) / (2 * eq)).max()),
                    float((np.abs(got["qvalues"].astype(np.float64) - r["qvalues"]) / (2 * eqv)).max()))
        print(f"{ctx}: {share:.4f} of 2 E against the reference")
        assert share <= 1.0, ctx
        assert np.array_equal(np.argmax(got["qvalues"], axis=1), np.argmax(r["qvalues"], axis=1)), ctx
        if mode == "train":
            continue                                                             # (the module draws its own noise: test 7)
        net = to_net(torch, s)
        res = net.quantiles(torch.from_numpy(x).to(DEV), taus=torch.from_numpy(r["taus"]).to(DEV), cos=True)
        for k, v in (("quantiles", res.quantiles), ("qvalues", res.qvalues), ("cos", res.cos)):
            FC.same_bits(v.cpu().numpy(), got[k], k + " through IQN.quantiles", ctx)
        FC.same_bits(res.taus.cpu().numpy().reshape(got["taus"].shape), got["taus"], "taus through IQN.quantiles", ctx)
        qv = net.get_qvalues(torch.from_numpy(x).to(DEV), taus=torch.from_numpy(r["taus"]).to(DEV))
        FC.same_bits(qv.cpu().numpy(), got["qvalues"], "get_qvalues", ctx)
        assert not qv.requires_grad and not res.quantiles.requires_grad


# ------------------------------------------------------------------------------------------------------------- 2: shapes
# (L, D, N, A, rows): every value of an axis meets small and large values of the others; rows N L^2 <= 2^24
SHAPES = [
    (1, 1, 1, 1, 1), (1, 875, 64, 64, 257), (1, 3, 12, 5, 9), (1, 64, 2, 2, 65), (1, 65, 13, 63, 7), (1, 63, 1, 4, 8),
    (31, 63, 13, 63, 7), (31, 1, 1, 4, 257), (31, 875, 2, 1, 8), (31, 65, 64, 2, 9), (31, 3, 12, 64, 1), (31, 64, 2, 5, 65),
    (32, 64, 12, 4, 65), (32, 3, 64, 64, 1), (32, 65, 1, 5, 257), (32, 875, 13, 2, 7), (32, 1, 2, 63, 9), (32, 63, 12, 1, 8),
    (33, 65, 13, 5, 9), (33, 1, 2, 63, 257), (33, 63, 64, 1, 65), (33, 875, 12, 4, 8), (33, 3, 1, 2, 7), (33, 64, 13, 64, 1),
    (250, 875, 12, 4, 8), (250, 1, 1, 1, 257), (250, 3, 64, 63, 1), (250, 64, 2, 64, 65), (250, 63, 13, 5, 7), (250, 65, 12, 2, 9),
    (256, 875, 1, 64, 9), (256, 64, 64, 1, 1), (256, 3, 13, 4, 8), (256, 65, 2, 5, 65), (256, 1, 12, 63, 7), (256, 63, 2, 2, 1),
    (64, 875, 8, 4, 257), (5, 7, 2, 3, 9), (96, 65, 5, 4, 65), (224, 64, 12, 5, 9),
]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(str(v) for v in s) for s in SHAPES])
def test_shapes_bit_for_bit(torch_cuda, shape):
    L, D, Nq, A, B = shape
    assert B * Nq * L * L <= 1 << 24
    rng = np.random.default_rng(hash(shape) & 0xFFFF)
    w = FC.random_weights(rng, D, L, A)
    taus = rng.random(size=(B, Nq)).astype(np.float32)
    for x in (rng.normal(size=(B, D)).astype(np.float32), (rng.random(size=(B, D)) < 0.3).astype(np.uint8) * rng.integers(1, 256, size=(B, D)).astype(np.uint8)):
        got = abi_forward(torch_cuda, w, x, Nq, taus=taus)
        check_bits(got, w, x, f"{shape} {x.dtype}", taus=taus)


# ------------------------------------------------------------------------------------------------------------- 3: strides and alignment
def test_strides_alignment_optional_outputs_and_guards(torch_cuda):
    rng = np.random.default_rng(11)
    D, L, Nq, A, B = 65, 33, 13, 5, 9
    w = FC.random_weights(rng, D, L, A)
    x = rng.normal(size=(B, D)).astype(np.float32)
    taus = rng.random(size=(B, Nq)).astype(np.float32)
    base = abi_forward(torch_cuda, w, x, Nq, taus=taus)
    check_bits(base, w, x, "base", taus=taus)

    def same(got, ctx):
        for k in OUTPUTS:
            if got[k] is not None:
                FC.same_bits(got[k], base[k], k, ctx)

    same(abi_forward(torch_cuda, w, x, Nq, taus=taus, stride=D + 7), "a state_stride above D")
    same(abi_forward(torch_cuda, w, x.astype(np.float32), Nq, taus=taus, stride=D + 1), "an odd state_stride")
    for name in FC.WEIGHTS + OUTPUTS + ("workspace",):
        same(abi_forward(torch_cuda, w, x, Nq, taus=taus, off=(name,)), f"{name} one element off a 16-byte boundary")
    same(abi_forward(torch_cuda, w, x, Nq, taus=taus, off=FC.WEIGHTS + OUTPUTS + ("workspace",)), "everything off")
    for name in OUTPUTS:
        got = abi_forward(torch_cuda, w, x, Nq, taus=taus, skip=(name,))
        assert got[name] is None
        same(got, f"{name} is NULL")
    same(abi_forward(torch_cuda, w, x, Nq, taus=taus, skip=("quantiles", "taus", "cos")), "qvalues alone")
    same(abi_forward(torch_cuda, w, x, Nq, taus=taus, skip=("qvalues", "taus", "cos")), "quantiles alone")
    abi_forward(torch_cuda, w, x[:0], Nq, taus=taus[:0], untouched=True)           # n == 0 launches nothing and writes nothing


# ------------------------------------------------------------------------------------------------------------- 4: position independence
def test_a_row_does_not_depend_on_the_batch(torch_cuda):
    rng = np.random.default_rng(12)
    D, L, Nq, A, B = 4, 8, 2, 2, 65537
    w = FC.random_weights(rng, D, L, A)
    x = rng.normal(size=(B, D)).astype(np.float32)
    key = dict(seed=0xABCDEF0123, first_env=5, epoch=2, turn=9, num_envs=B, agent0=3)
    one = abi_forward(torch_cuda, w, x, Nq, key=key)
    two = abi_forward(torch_cuda, w, x, Nq, key=key)
    for k in OUTPUTS:
        FC.same_bits(one[k], two[k], k, "twice")
    FC.same_bits(one["taus"], FC.keyed_taus(key["seed"], 5, np.arange(B), np.full(B, 3), 2, 9, Nq), "keyed taus")
    for row in (0, 1, 4095, 65536):
        alone = abi_forward(torch_cuda, w, x[row:row + 1], Nq, key=dict(key, first_env=5 + row))      # the same key: env = first_env + row
        for k in OUTPUTS:
            FC.same_bits(alone[k][0], one[k][row], k, f"row {row} alone")
    sample = np.r_[0:70, 4090:4100, 65500:65537]
    check_bits({k: v[sample] for k, v in one.items()}, w, x[sample], "a sample of the rows")


# ------------------------------------------------------------------------------------------------------------- 5: NaN
def test_a_nan_stays_in_its_row(torch_cuda):
    rng = np.random.default_rng(13)
    D, L, Nq, A, B = 7, 33, 12, 4, 11
    w = FC.random_weights(rng, D, L, A)
    x = rng.normal(size=(B, D)).astype(np.float32)
    taus = rng.random(size=(B, Nq)).astype(np.float32)
    clean = abi_forward(torch_cuda, w, x, Nq, taus=taus)
    x2 = x.copy()
    x2[6, 3] = np.nan
    got = abi_forward(torch_cuda, w, x2, Nq, taus=taus)
    others = np.arange(B) != 6
    for k in OUTPUTS:
        FC.same_bits(got[k][others], clean[k][others], k, "the rows beside the NaN")
    check_bits(got, w, x2, "with a NaN", taus=taus)
    assert np.isnan(got["qvalues"][6]).any() and not np.isnan(got["cos"]).any()
    x3 = x.copy()
    x3[2, 0] = np.inf
    check_bits(abi_forward(torch_cuda, w, x3, Nq, taus=taus), w, x3, "with an infinity", taus=taus)


# ------------------------------------------------------------------------------------------------------------- 6: keyed taus
def test_keyed_taus(torch_cuda):
    rng = np.random.default_rng(14)
    D, L, Nq, A, E = 3, 5, 13, 3, 7
    B = 3 * E                                                                    # three agents' rows, agent-major
    w = FC.random_weights(rng, D, L, A)
    x = rng.normal(size=(B, D)).astype(np.float32)
    key = dict(seed=(1 << 63) + 12345, first_env=(1 << 32) + 9, epoch=5, turn=77, num_envs=E, agent0=2)
    got = abi_forward(torch_cuda, w, x, Nq, key=key)
    rows = np.arange(B)
    want = FC.keyed_taus(key["seed"], key["first_env"], rows % E, 2 + rows // E, 5, 77, Nq)
    check_bits(got, w, x, "keyed", taus=want)
    for change in (dict(agent0=3), dict(turn=78), dict(epoch=6), dict(seed=key["seed"] + 1)):
        other = abi_forward(torch_cuda, w, x, Nq, key=dict(key, **change))["taus"]
        assert not np.array_equal(other, got["taus"]) and len(np.unique(other)) == other.size, change
    FC.same_bits(abi_forward(torch_cuda, w, x, Nq, key=dict(key, agent0=3))["taus"][:2 * E], got["taus"][E:], "taus", "agent0 + 1 is the next agent's rows")
    idx = rng.permutation(B).astype(np.int64) + 2 * E                            # the same (env, agent) pairs in another order
    re = abi_forward(torch_cuda, w, x, Nq, key=dict(key, agent0=0), idx=idx)
    FC.same_bits(re["taus"], got["taus"][idx - 2 * E], "taus", "idx reorders the keys")
    check_bits(re, w, x, "idx")
    idx[4] = -1
    idx[5] = E * 128
    bad = abi_forward(torch_cuda, w, x, Nq, key=dict(key, agent0=0), idx=idx)
    assert np.isnan(bad["taus"][[4, 5]]).all() and np.isnan(bad["qvalues"][[4, 5]]).all()
    keep = np.ones(B, bool)
    keep[[4, 5]] = False
    for k in OUTPUTS:
        FC.same_bits(bad[k][keep], re[k][keep], k, "the rows beside a key that names no pair")


# ------------------------------------------------------------------------------------------------------------- 7: training mode
def test_training_mode_passes_the_noisy_effective_weights(torch_cuda):
    torch = torch_cuda
    s = SETS["65_33_13_5_9"]
    net = to_net(torch, s, "train")
    x = torch.from_numpy(s["states"]).to(DEV)
    taus = torch.from_numpy(s["train"]["taus"]).to(DEV)
    before = net.ff_1.epsilon_weight.clone()
    res = net.quantiles(x, taus=taus, cos=True)
    assert not torch.equal(before, net.ff_1.epsilon_weight)                      # fresh noise, as NoisyLinear.forward draws it
    sd = {k: v.cpu().numpy() for k, v in net.state_dict().items()}
    w = FC.effective_of(sd, True)                                                # weight + sigma * epsilon of the module's buffers
    assert not np.array_equal(w["w_ff"], sd["ff_1.weight"])
    quant, qv = FC.restate(w, s["states"], res.cos.cpu().numpy())
    FC.same_bits(res.quantiles.cpu().numpy(), quant, "quantiles in training mode")
    FC.same_bits(res.qvalues.cpu().numpy(), qv, "qvalues in training mode")
    net.eval()
    calm = net.quantiles(x, taus=taus)
    assert not torch.equal(calm.quantiles, res.quantiles)
    FC.same_bits(calm.quantiles.cpu().numpy(), FC.restate(FC.effective_of(sd, False), s["states"], res.cos.cpu().numpy())[0], "eval mode again")


# ------------------------------------------------------------------------------------------------------------- 8: a recorded graph
def test_recorded_graph_replays_on_new_states_and_weights(torch_cuda):
    torch = torch_cuda
    from sorrel_amd.models import iqn as M

    s = SETS["65_33_13_5_9"]
    net = to_net(torch, s)
    x = torch.from_numpy(s["states"]).to(DEV)
    taus = torch.from_numpy(s["eval"]["taus"]).to(DEV)
    out = M.IQNOutput(s["B"], s["N"], s["A"], s["L"], DEV, cos=True)
    net.get_qvalues(x, taus=taus, out=out, cos=True)                             # (code objects loaded before the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert net.get_qvalues(x, taus=taus, out=out, cos=True) is out.qvalues
    rng = np.random.default_rng(15)
    x.copy_(torch.from_numpy(rng.normal(size=s["states"].shape).astype(np.float32)))
    with torch.no_grad():
        net.ff_1.weight.mul_(0.5)
        net.head1.bias.add_(0.25)
    out.qvalues.zero_()
    graph.replay()
    torch.cuda.synchronize()
    w = FC.effective_of({k: v.cpu().numpy() for k, v in net.state_dict().items()}, False)
    quant, qv = FC.restate(w, x.cpu().numpy(), out.cos.cpu().numpy())
    FC.same_bits(out.quantiles.cpu().numpy(), quant, "quantiles after the replay")
    FC.same_bits(out.qvalues.cpu().numpy(), qv, "qvalues after the replay")
    eager = net.quantiles(x, taus=taus)
    assert torch.equal(eager.quantiles, out.quantiles)


# ------------------------------------------------------------------------------------------------------------- 9: a policy turn
def test_policy_turn_with_iqn_actor_eager_against_recorded(torch_cuda):
    torch = torch_cuda
    from sorrel_amd.models import iqn as M
    from tests.gpu_common import make_env

    E, A, T = 64, 2, 3

    def build():
        made = []

        def factory(input_size, action_space):
            torch.manual_seed(100 + len(made))
            made.append(M.IQNActor(input_size, action_space, layer_size=33, n_quantiles=5, seed=100 + len(made), memory_size=8, num_envs=E, device=DEV))
            return made[-1]

        env = make_env(8, 8, A, 2, E, p=0.05, seed=23, model_factory=factory)
        for a, agent in enumerate(env.agents):
            agent.model.bind(env, a)
        return env

    eager, rec = build(), build()
    for a in range(A):
        for p, q in zip(eager.agents[a].model.net.parameters(), rec.agents[a].model.net.parameters()):
            assert torch.equal(p, q)
    cap = rec.capture_turn(warmup=1, force=True)
    assert cap is not None, rec.capture_error
    seen = []
    for t in range(T):
        eager.take_turn()
        if t >= 1:
            rec.take_turn()
        torch.cuda.synchronize()
        for a in range(A):
            te, tr = eager.agents[a].model._out.taus, rec.agents[a].model._out.taus
            assert torch.equal(te, tr), (t, a)
            want = FC.keyed_taus(int(eager._engine.spec.seed), eager._engine.first_env_id, np.arange(E), np.full(E, a), eager.epoch, t + 1, 5)
            FC.same_bits(te.cpu().numpy().reshape(E, 5), want, "taus of the turn", (t, a))
        seen.append(eager.agents[0].model._out.taus.clone())
        assert torch.equal(eager.actions, rec.actions), t
        for name in ("grid", "agent_pos", "total_reward"):
            assert torch.equal(getattr(eager.world, name), getattr(rec.world, name)), (t, name)
    assert cap.turns_replayed == T - 1
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])     # a replayed turn draws its own taus
    eager.raise_on_status()
    rec.raise_on_status()
