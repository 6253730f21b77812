"""IQN's network forward without a GPU: ``fmaf`` restated in NumPy against libm's; the NumPy restatement of ``sgw_iqn_forward``'s semantics
(``tests/iqn_forward_common.py``) and ``IQN.forward`` on the CPU against what the reference's ``IQN`` computed
(``tests/golden/iqn_forward``) -- ``IQN.forward`` gives the reference's bits in eval mode --; a reference ``state_dict`` loading into
``IQN``; the layout of ``sgw_iqn_forward_desc`` against gcc; every descriptor the call rejects (validation precedes the launch, so no
device is needed) and what the Python wrappers refuse; the keyed taus against a NumPy Philox; the header / ``EXPORTS`` agreement."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import gridstep_oracle as O
from sorrel_amd import _native as N
from sorrel_amd.models import iqn as M
from tests import helpers as H
from tests import learner_common as LK
from tests import iqn_forward_common as FC

SETS = FC.load_fixture()
TAGS = sorted(SETS)


# ------------------------------------------------------------------------------------------------------------- fmaf
def test_fmaf_restated_equals_libm():
    libm = FC.libm_fmaf()
    one = np.float32(1 + 2.0 ** -23)
    small = np.float32((1 - 2.0 ** -23) * 2.0 ** -24)
    # plain float64 arithmetic rounds these two twice and misses; one rounding gives 0x3F800001 for both, and so does libm
    for b in (small, -small):
        got = FC.fmaf(one, b, one)
        want = np.float32(libm(float(one), float(b), float(one)))
        assert FC.bits(got.reshape(1))[0] == FC.bits(want.reshape(1))[0] == 0x3F800001, (b, got, want)
        naive = np.float32(np.float64(one) * np.float64(b) + np.float64(one))
        assert FC.bits(naive.reshape(1))[0] != 0x3F800001                                         # (the case is a real one)
    rng = np.random.default_rng(5)
    n = 20000
    a = (rng.normal(size=n) * 2.0 ** rng.integers(-30, 30, size=n)).astype(np.float32)
    b = (rng.normal(size=n) * 2.0 ** rng.integers(-30, 30, size=n)).astype(np.float32)
    c = (rng.normal(size=n) * 2.0 ** rng.integers(-40, 40, size=n)).astype(np.float32)
    c[: n // 4] = (-(a[: n // 4].astype(np.float64) * b[: n // 4])).astype(np.float32)           # cancellation: the residual decides
    got = FC.fmaf(a, b, c)
    want = np.array([libm(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)
    FC.same_bits(got, want, "fmaf")
    assert FC.fmaf(np.float32(0), np.float32(-0.0), np.float32(-0.0)).view(np.uint32) == 0x80000000   # the kernel's k padding: -0 stays -0
    assert np.isnan(FC.fmaf(np.float32(np.inf), np.float32(0), np.float32(1)))


# ------------------------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("tag", TAGS)
def test_restatement_lies_within_the_bound_of_the_reference(tag):
    s = SETS[tag]
    for mode in ("eval", "u8", "train"):
        r = s[mode]
        x = s["states_u8"] if mode == "u8" else s["states"]
        quant, qv = FC.restate(r["w"], x, r["cos"])
        q64, qv64, eq, eqv = FC.bound(r["w"], x, r["cos"])
        assert np.abs(q64 - r["quantiles64"]).max() <= 1e-9 * (1 + np.abs(q64).max())
        assert (np.abs(quant.astype(np.float64) - r["quantiles"]) <= 2 * eq).all(), (tag, mode)
        assert (np.abs(qv.astype(np.float64) - r["qvalues"]) <= 2 * eqv).all(), (tag, mode)
        assert np.array_equal(np.argmax(qv, axis=1), np.argmax(r["qvalues"], axis=1)), (tag, mode)
        # the cosine's argument is the float32 product with the rounded constants
        assert np.array_equal(FC.cos_args(r["taus"]), (r["taus"] * FC.pis()[None, None, :]).astype(np.float32))


def _net(s, mode="eval"):
    net = M.IQN((s["D"],), s["A"], s["L"], seed=0, n_quantiles=s["N"], n_frames=1)
    missing = net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in s["sd"].items()})       # the reference's names and shapes
    assert not missing.missing_keys and not missing.unexpected_keys
    net.train(mode == "train")
    return net


@pytest.mark.parametrize("tag", TAGS)
def test_a_reference_state_dict_loads_and_forward_gives_the_reference_bits(tag, monkeypatch):
    s = SETS[tag]
    net = _net(s)
    assert sorted(net.state_dict()) == sorted(s["sd"])
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                      # the generator's setting: a BLAS splits its sums by the threads it has
    try:
        _forward_gives_the_reference_bits(s, net, tag, monkeypatch)
    finally:
        torch.set_num_threads(threads)


def _forward_gives_the_reference_bits(s, net, tag, monkeypatch):
    for mode in ("eval", "u8"):
        r = s[mode]
        x = torch.from_numpy(s["states_u8"]).float() if mode == "u8" else torch.from_numpy(s["states"])
        monkeypatch.setattr(torch, "rand", lambda *shape, **kw: torch.from_numpy(r["taus"]).reshape(shape))
        with torch.no_grad():
            quant, taus = net(x, s["N"])
            qv = net.get_qvalues(x)
        FC.same_bits(taus.numpy(), r["taus"], "taus", tag)
        FC.same_bits(quant.numpy(), r["quantiles"], "quantiles", tag + mode)
        FC.same_bits(qv.numpy(), r["qvalues"], "qvalues", tag + mode)
    # the effective weights of eval mode are the parameters; of training mode weight + sigma * epsilon of the buffers
    for got, want in zip(net.effective_weights(), (s["eval"]["w"][k] for k in FC.WEIGHTS)):
        FC.same_bits(got.numpy().reshape(want.shape), want, "effective weights", tag)
    net.train(True)
    for got, want in zip(net.effective_weights(resample=False), (s["train"]["w"][k] for k in FC.WEIGHTS)):
        FC.same_bits(got.numpy().reshape(want.shape), want, "noisy effective weights", tag)
    before = net.ff_1.epsilon_weight.clone()
    net.effective_weights()
    assert not torch.equal(before, net.ff_1.epsilon_weight) or before.numel() < 2                        # fresh noise per call, as forward draws it


def test_iqn_on_cpu_tensors_and_autograd():
    s = SETS["7_5_2_3_9"]
    net = _net(s)
    x = torch.from_numpy(s["states"])
    taus = torch.from_numpy(s["eval"]["taus"])
    res = net.quantiles(x, taus=taus, cos=True)
    FC.same_bits(res.quantiles.numpy(), s["eval"]["quantiles"], "quantiles by torch ops")
    FC.same_bits(res.cos.numpy(), s["eval"]["cos"], "cos")
    assert net.quantiles(x, taus=taus, out=res) is res and not res.quantiles.requires_grad
    assert tuple(net.get_qvalues(torch.from_numpy(s["states_u8"]), taus=taus).shape) == (s["B"], s["A"])
    quant, _ = net(x.clone().requires_grad_(True), s["N"])
    quant.sum().backward()
    assert net.head1.weight.grad is not None and net.ff_1.sigma_weight.grad is None      # eval mode: the mean weights only
    net.train(True)
    quant, _ = net(x, s["N"])
    quant.sum().backward()
    assert net.ff_1.sigma_weight.grad is not None and net.ff_1.sigma_weight.grad.abs().sum() > 0
    actor = M.IQNActor((s["D"],), s["A"], layer_size=s["L"], n_quantiles=s["N"])
    assert tuple(actor.take_action(x).shape) == (s["B"], s["A"]) and actor.train_step() == 0.0 and not hasattr(actor, "optimizer")


def test_wrappers_refuse(built):
    s = SETS["7_5_2_3_9"]
    net = _net(s)
    x = torch.from_numpy(s["states"])
    with pytest.raises(TypeError):
        net.quantiles(x.double())
    with pytest.raises(TypeError):
        net.quantiles(s["states"])
    with pytest.raises(ValueError, match="head layer"):
        net.quantiles(x[:, :-1])
    with pytest.raises(ValueError, match="quantiles"):
        net.quantiles(x, 65)
    with pytest.raises(ValueError, match="taus"):
        net.quantiles(x, taus=torch.zeros(s["B"], s["N"] + 1))
    with pytest.raises(TypeError):
        net.quantiles(x, taus=torch.zeros(s["B"], s["N"], dtype=torch.float64))
    with pytest.raises(TypeError):
        net.quantiles(x, out=object())
    other = M.IQNOutput(s["B"] + 1, s["N"], s["A"], s["L"], "cpu")
    with pytest.raises(ValueError, match="out="):
        net.quantiles(x, out=other)
    with pytest.raises(ValueError, match="out="):
        net.quantiles(x, out=M.IQNOutput(s["B"], s["N"], s["A"], s["L"], "cpu"), cos=True)
    wide = M.IQN((3,), 65, 4, seed=0, n_quantiles=2, n_frames=1)
    with pytest.raises(ValueError, match="actions"):
        wide.quantiles(torch.zeros(2, 3))
    big = M.IQN((3,), 2, 257, seed=0, n_quantiles=2, n_frames=1)
    with pytest.raises(ValueError, match="layer_size"):
        big.quantiles(torch.zeros(2, 3))


# ------------------------------------------------------------------------------------------------------------- keyed taus
def test_keyed_taus_are_the_oracles_philox():
    seed, first_env, epoch, turn, N_ = 0x1234567890ABCDEF, 7, 3, 5, 13
    env, agent = np.array([0, 1, 64, 65]), np.array([0, 2, 127, 5])
    taus = FC.keyed_taus(seed, first_env, env, agent, epoch, turn, N_)
    assert taus.dtype == np.float32 and taus.shape == (4, N_) and (taus >= 0).all() and (taus < 1).all()
    for r in range(4):
        for q in range(N_):
            u = int(O.rng_u32(seed, first_env + int(env[r]), epoch, turn, FC.STREAM_TAU, (int(agent[r]) << 6) | q))
            assert taus[r, q] == np.float32((u >> 8) * 2.0 ** -24)
    # a function of every part of the key
    base = FC.keyed_taus(seed, first_env, env, agent, epoch, turn, N_)
    for change in (dict(seed=seed + 1), dict(first_env=first_env + 1), dict(epoch=epoch + 1), dict(turn=turn + 1), dict(agent=agent + 1)):
        kw = dict(seed=seed, first_env=first_env, env=env, agent=agent, epoch=epoch, turn=turn, N=N_)
        kw.update(change)
        assert not np.array_equal(base, FC.keyed_taus(**kw)), change
    assert len(np.unique(base)) == base.size


# ------------------------------------------------------------------------------------------------------------- header and binding
def test_header_declares_the_entry_points_and_the_binding_mirrors_them(built):
    text = open(os.path.join(H.ROOT, "include", "sgw.h")).read()
    assert re.search(r"int sgw_iqn_forward\(const sgw_iqn_forward_desc\* desc, void\* stream\);", text)
    assert re.search(r"int64_t sgw_iqn_forward_workspace_bytes\(int64_t n, int32_t layer_size\);", text)
    assert re.search(r"int sgw_turn_iqn_forward\(sgw_engine\* eng, int32_t agent, const sgw_iqn_forward_desc\* desc, void\* stream\);", text)
    macros = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+(SGW_[A-Z_0-9]+)\s+(0x[0-9A-Fa-f]+|\d+)u?\b", text)}
    assert N.STREAM_TAU == macros["SGW_STREAM_TAU"] == FC.STREAM_TAU == 11
    assert len({v for k, v in macros.items() if k.startswith("SGW_STREAM_")}) == 12                  # every stream has a number of its own
    lib = N.load()
    assert lib.sgw_version() == b"sgw 0.3 (gfx950)"                            # the additions are append-only
    wb = lib.sgw_iqn_forward_workspace_bytes
    assert wb(0, 250) == 0 and wb(1, 1) == 4 and wb(65536, 250) == 65536 * 250 * 4
    assert wb(-1, 250) == N.EINVAL and b"n =" in lib.sgw_last_error()
    assert wb(4, 0) == N.EINVAL and wb(4, 257) == N.EINVAL and b"layer_size" in lib.sgw_last_error()
    assert wb((1 << 63) - 1, 256) == N.EINVAL                                  # (no overflow)


# ------------------------------------------------------------------------------------------------------------- refusals
POINTERS = ("states",) + FC.WEIGHTS


def good_desc():
    """A descriptor the call accepts (the pointers are never followed: every test below is rejected, or has n == 0)."""
    d = N.SgwIqnForwardDesc()
    for name in POINTERS:
        setattr(d, name, 4096)
    d.out_qvalues = d.out_quantiles = d.out_taus = d.out_cos = d.workspace = 8192
    d.workspace_bytes = 1 << 20
    d.n, d.state_stride, d.num_envs = 0, 875, 8
    d.in_features, d.layer_size, d.num_quantiles, d.num_actions, d.n_cos = 875, 250, 12, 4, 64
    return d


REJECTED = [(f"{name} is NULL", {name: None}, b"must not be NULL") for name in POINTERS] + [
    ("neither out_qvalues nor out_quantiles", {"out_qvalues": None, "out_quantiles": None}, b"out_qvalues"),
    ("n < 0", {"n": -1}, b"n ="),
    ("in_features < 1", {"in_features": 0}, b"in_features"),
    ("layer_size < 1", {"layer_size": 0}, b"layer_size"),
    ("layer_size > 256", {"layer_size": 257}, b"layer_size"),
    ("num_quantiles < 1", {"num_quantiles": 0}, b"num_quantiles"),
    ("num_quantiles > 64", {"num_quantiles": 65}, b"num_quantiles"),
    ("num_actions < 1", {"num_actions": 0}, b"num_actions"),
    ("num_actions > 64", {"num_actions": 65}, b"num_actions"),
    ("n_cos != 64", {"n_cos": 32}, b"n_cos"),
    ("unknown state_type", {"state_type": 2}, b"state_type"),
    ("negative state_type", {"state_type": -1}, b"state_type"),
    ("state_stride < in_features", {"state_stride": 874}, b"state_stride"),
    ("reserved0 set", {"reserved0": 1}, b"reserved"),
    ("reserved1 set", {"reserved1": 1}, b"reserved"),
    ("num_envs < 1 where taus are drawn", {"num_envs": 0}, b"num_envs"),
    ("epoch >= 2^28", {"epoch": 1 << 28}, b"epoch"),
    ("negative agent key", {"agent0": -1}, b"agents"),
    ("agent key past the last", {"agent0": 127, "num_envs": 4}, b"agents"),
    ("misaligned float32 states", {"states": 4098}, b"states"),
] + [(f"misaligned {name}", {name: 4098}, b"float32") for name in FC.WEIGHTS + ("taus", "out_qvalues", "out_quantiles", "out_taus", "out_cos", "workspace")] + [
    ("misaligned idx", {"idx": 4100}, b"idx"),
    ("no workspace", {"workspace": None}, b"workspace"),
    ("a workspace that is too small", {"workspace_bytes": 5 * 250 * 4 - 1}, b"workspace"),
    ("offsets past 64 bits", {"n": 1 << 50, "state_stride": 1 << 20, "taus": 4096}, b"64-bit"),
    ("offsets past 64 bits in the outputs", {"n": 1 << 48, "taus": 4096}, b"64-bit"),
]


@pytest.mark.parametrize("case", REJECTED, ids=[c[0] for c in REJECTED])
def test_sgw_iqn_forward_rejects(built, case):
    _, change, word = case
    d = good_desc()
    d.n = 5                                       # (a call that would launch, were it accepted)
    LK.assert_rejected(N.load().sgw_iqn_forward, d, change, word)


def test_sgw_iqn_forward_null_desc_and_no_rows(built):
    lib = N.load()
    assert lib.sgw_iqn_forward(None, None) == N.EINVAL and b"desc is NULL" in lib.sgw_last_error()
    assert lib.sgw_turn_iqn_forward(None, 0, None, None) == N.EINVAL and b"NULL engine" in lib.sgw_last_error()
    d = good_desc()
    assert lib.sgw_iqn_forward(C.byref(d), None) == N.OK                         # n == 0: nothing is launched
    d.out_quantiles = d.out_taus = d.out_cos = None                              # optional outputs
    d.workspace, d.workspace_bytes = None, 0                                     # no rows need no workspace
    d.states, d.state_type = 4097, 1                                             # uint8 states need no alignment
    d.taus, d.num_envs, d.epoch, d.agent0 = 4096, 0, 1 << 30, -5                 # given taus need no key
    d.layer_size, d.num_quantiles, d.num_actions, d.in_features, d.state_stride = 256, 64, 64, 1, 1
    assert lib.sgw_iqn_forward(C.byref(d), None) == N.OK
    d.out_qvalues, d.out_quantiles = None, 8192
    d.layer_size = d.num_quantiles = d.num_actions = 1
    assert lib.sgw_iqn_forward(C.byref(d), None) == N.OK
