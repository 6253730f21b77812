"""CPU tests of the IQN learner (``sorrel_amd.models.PyTorchIQN`` = ``models.iqn_learner.iRainbowModel``): its torch path against the
fixture of the reference's own ``iRainbowModel.train_step`` (bit for bit, each step from its recorded before-state), the gate, the epoch
hooks, the checkpoint layout, the drop-in import, and that it learns."""
import inspect

import numpy as np
import pytest
import torch

from tests import iqn_learner_common as LC
from tests import learner_common as LK

CASES = [(LC.tag_of(shape), k) for shape in LC.SHAPES for k in range(LC.STEPS)]


def eval_loss(model, args):
    """The loss of a batch with the mean weights and the given taus, computed on the CPU from copies of both networks."""
    from sorrel_amd.losses import _iqn_loss_torch

    cpu = LC.make_model((model.qnetwork_local.head1.in_features // model.n_frames, model.n_frames, model.layer_size, model.n_quantiles,
                         model.action_space, model.batch_size), "cpu")
    cpu.qnetwork_local.load_state_dict({k: v.cpu() for k, v in model.qnetwork_local.state_dict().items()})
    cpu.qnetwork_target.load_state_dict({k: v.cpu() for k, v in model.qnetwork_target.state_dict().items()})
    states, actions, rewards, next_states, dones, valid = (x.cpu() for x in args["batch"])
    taus = [t.cpu() for t in args["taus"]]
    with torch.no_grad():
        n = cpu.n_quantiles
        a, _ = cpu.qnetwork_local.forward_flat(next_states, n, taus[0], noise=False)
        b, _ = cpu.qnetwork_target.forward_flat(next_states, n, taus[1], noise=False)
        c, t = cpu.qnetwork_local.forward_flat(states, n, taus[2], noise=False)
        return float(_iqn_loss_torch(c, t, a, b, actions, rewards, dones, valid, cpu.GAMMA ** cpu.n_step)[0])


def test_fixture_is_data_only_and_small():
    import os

    assert os.path.getsize(LC.FIXTURE) < os.path.getsize(os.path.join(LC.H.ROOT, "tests", "golden", "iqn_forward", "forward.npz"))
    with np.load(LC.FIXTURE, allow_pickle=False) as data:
        assert all(data[k].dtype.kind in "fiuU" for k in data.files)
    fixture = LC.load_fixture()
    assert sorted(fixture) == sorted(LC.tag_of(s) for s in LC.SHAPES)
    for case in fixture.values():
        assert len(case["snaps"]) == LC.STEPS + 1 and len(case["steps"]) == LC.STEPS and len(case["param_names"]) == 16 and len(case["sd_names"]) == 22
        assert not case["snaps"][0]["exp_avg"] and len(case["snaps"][1]["exp_avg"]) == 16


@pytest.mark.parametrize("tag, k", CASES)
def test_torch_path_reproduces_the_reference_bit_for_bit(tag, k):
    case = LC.load_fixture()[tag]
    rec = case["steps"][k]
    model = LC.fill_memory(LC.put_state(LC.make_model(case["shape"], "cpu"), case["snaps"][k]))
    assert model.qnetwork_local.training and model.qnetwork_target.training        # the reference never puts either into eval mode
    loss = model.train_step(**LC.step_args(rec, "cpu"))
    assert isinstance(loss, np.ndarray) and loss.shape == ()
    LK.same_bits(loss, rec["loss"], "loss", (tag, k))
    LC.same_state(LC.get_state(model), case["snaps"][k + 1], ctx=(tag, k))
    for part in ("local", "target"):                                               # and so it holds the device path's cap with d_r = d_ref
        for name in case["param_names"]:
            p64 = rec["after64"][part][name]
            assert LC.distance(getattr(model, "qnetwork_" + part).state_dict()[name].numpy(), p64) <= 0.5 * LC.cap(rec["d_ref"][f"{part}/{name}"], p64)


def test_constructor_is_the_references():
    from sorrel_amd.models import PyTorchIQN, iRainbowModel

    assert PyTorchIQN is iRainbowModel
    params = inspect.signature(PyTorchIQN.__init__).parameters
    names = [n for n in params if n != "self"]
    assert names == ["input_size", "action_space", "layer_size", "epsilon", "device", "seed", "n_frames", "n_step", "sync_freq", "model_update_freq",
                     "batch_size", "memory_size", "LR", "TAU", "GAMMA", "n_quantiles", "num_envs"]
    defaults = {n: p.default for n, p in params.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(n_step=3, sync_freq=200, model_update_freq=4, batch_size=64, memory_size=1024, LR=0.001, TAU=0.001, GAMMA=0.99,
                            n_quantiles=12, num_envs=1)


def test_attributes():
    from sorrel_amd.buffers import Buffer
    from sorrel_amd.models.iqn import IQN
    from sorrel_amd.optim import FusedAdam

    m = LC.make_model(LC.SHAPES[1], "cpu", num_envs=3)
    assert isinstance(m.qnetwork_local, IQN) and isinstance(m.qnetwork_target, IQN) and m.qnetwork_local is not m.qnetwork_target
    assert m.models == {"local": m.qnetwork_local, "target": m.qnetwork_target}
    assert isinstance(m.optimizer, FusedAdam) and m.optimizer.max_grad_norm == 1.0 and m.optimizer.tau == m.TAU
    assert isinstance(m.memory, Buffer) and m.memory.n_frames == 5 and m.memory.num_envs == 3 and m.memory.obs_shape == (7,)
    assert str(m) == "iRainbowModel(input_size=35,action_space=5)"
    for p, q in zip(m.qnetwork_local.parameters(), m.qnetwork_target.parameters()):
        assert torch.equal(p, q)
    m.set_epsilon(0.5)
    m.epsilon_decay(0.1)
    assert m.epsilon == pytest.approx(0.45)


def test_gate_leaves_everything_untouched_and_returns_zero():
    m = LC.make_model(LC.SHAPES[0], "cpu")
    LC.fill_memory(m, rows=m.batch_size)                   # len(memory) == batch_size: not above it
    before = LC.get_state(m)
    loss = m.train_step()
    assert isinstance(loss, np.ndarray) and loss.dtype == np.float32 and loss.shape == () and float(loss) == 0.0
    LC.same_state(LC.get_state(m), before)
    assert m.steps_done == 0
    LC.fill_memory(m, rows=1)
    loss = m.train_step()
    assert float(loss) != 0.0 and m.steps_done == 1
    assert any(not np.array_equal(a, before["local"][k]) for k, a in LC.get_state(m)["local"].items() if "epsilon" not in k)


def test_start_epoch_action_adds_the_empty_frames_and_syncs_on_the_right_epochs():
    m = LC.make_model(LC.SHAPES[1], "cpu", sync_freq=3)
    LC.fill_memory(m)
    for _ in range(2):
        m.train_step()
    differs = lambda: any(not torch.equal(p, q) for p, q in zip(m.qnetwork_local.parameters(), m.qnetwork_target.parameters()))  # noqa: E731
    assert differs()
    for epoch in (1, 2, 4, 5):
        idx, size = m.memory.idx, m.memory.size
        m.start_epoch_action(epoch=epoch)
        assert m.memory.idx == (idx + m.n_frames - 1) % m.memory.capacity and m.memory.size == min(size + 1, m.memory.capacity)
        assert differs(), epoch
    for epoch in (3, 0, 6):
        m.train_step()
        assert differs()
        m.start_epoch_action(epoch=epoch)
        assert not differs(), epoch
    m.end_epoch_action(epoch=0)


def test_soft_update_is_the_references_line():
    m = LC.make_model(LC.SHAPES[0], "cpu", TAU=0.25)
    with torch.no_grad():
        for p in m.qnetwork_local.parameters():
            p.add_(1.0)
    want = [0.25 * p.data + (1.0 - 0.25) * q.data for p, q in zip(m.qnetwork_local.parameters(), m.qnetwork_target.parameters())]
    m.soft_update()
    for q, w in zip(m.qnetwork_target.parameters(), want):
        assert torch.equal(q, w)


def test_save_then_load_round_trips_in_the_references_layout(tmp_path):
    case = LC.load_fixture()[LC.tag_of(LC.SHAPES[1])]
    m = LC.fill_memory(LC.put_state(LC.make_model(case["shape"], "cpu"), case["snaps"][2]))
    m.train_step()
    path = tmp_path / "checkpoints" / "epoch0-agent-0.pkl"
    m.save(path)
    ckpt = torch.load(path)
    assert sorted(ckpt) == ["local", "optim", "target"]
    assert list(ckpt["local"]) == case["sd_names"] and list(ckpt["target"]) == case["sd_names"]        # the reference's names, in its order
    assert sorted(ckpt["optim"]) == ["param_groups", "state"] and len(ckpt["optim"]["state"]) == 16
    other = LC.make_model(case["shape"], "cpu", seed=99)
    other.load(path)
    LC.same_state(LC.get_state(other), LC.get_state(m))
    # the reference's own file (its state_dicts and torch.optim.Adam's state, as the fixture recorded them) loads the same way
    snap = case["snaps"][3]
    names = case["param_names"]
    ref = dict(local={k: torch.from_numpy(v.copy()) for k, v in snap["local"].items()}, target={k: torch.from_numpy(v.copy()) for k, v in snap["target"].items()},
               optim=dict(state={i: dict(step=torch.tensor(3.0), exp_avg=torch.from_numpy(snap["exp_avg"][n].copy()),
                                         exp_avg_sq=torch.from_numpy(snap["exp_avg_sq"][n].copy())) for i, n in enumerate(names)},
                          param_groups=ckpt["optim"]["param_groups"]))
    torch.save(ref, tmp_path / "reference.pkl")
    other.load(tmp_path / "reference.pkl")
    LC.same_state(LC.get_state(other), snap)


def test_drop_in_import_gives_this_class():
    import sorrel_amd.compat as compat
    from sorrel_amd.models import PyTorchIQN

    assert "iqn_loss" in compat.OUT_OF_SCOPE["models.pytorch"] and "PyTorchIQN" in compat.OUT_OF_SCOPE["models.pytorch"]
    compat.install()
    try:
        from sorrel.models import PyTorchIQN as aliased

        assert aliased is PyTorchIQN
        with pytest.raises(ModuleNotFoundError, match="PyTorchIQN"):
            import sorrel.models.pytorch  # noqa: F401
    finally:
        compat.uninstall()


def test_take_action_uses_the_mean_weights_and_leaves_training_alone():
    m = LC.make_model(LC.SHAPES[1], "cpu")
    net = m.qnetwork_local
    with torch.no_grad():
        for name in ("ff_1", "advantage", "value"):
            getattr(net, name).sigma_weight.fill_(0.5)     # noise would show
    x = torch.randn(4, 35)
    torch.manual_seed(5)
    q = m.take_action(x)
    assert net.training and q.shape == (4, 5) and q.dtype == torch.float32 and not q.requires_grad
    torch.manual_seed(5)
    net.eval()
    want = net.get_qvalues(x).detach()
    net.train()
    assert torch.equal(q, want)


@pytest.mark.parametrize("training", (False, True), ids=("eval", "training"))
def test_the_torch_entry_points_agree_bit_for_bit(training, monkeypatch):
    """``forward``, ``forward_fused`` and ``quantiles`` on the CPU and the learner's network call (acting's in eval mode, the step's in
    training mode), with given taus and given noise."""
    case = LC.load_fixture()[LC.tag_of(LC.SHAPES[0])]
    args = LC.step_args(case["steps"][0], "cpu")
    x, taus, eps = args["batch"][0], args["taus"][2], args["noise"][12:18]
    B, N = taus.shape
    net = LC.put_state(LC.make_model(case["shape"], "cpu"), case["snaps"][0]).qnetwork_local.train(training)
    layers = (net.ff_1, net.advantage, net.value)

    def held():
        return [e for layer in layers for e in (layer.epsilon_weight, layer.epsilon_bias)]

    got = {}
    got["learner"] = net.forward_flat(x.view(B, -1), N, taus, noise=training, eps=eps if training else None)   # (copies eps into the layers)
    if training:
        assert all(torch.equal(a, b) for a, b in zip(held(), eps))
    monkeypatch.setattr(torch.Tensor, "normal_", lambda t, *a, **k: t)             # the other calls apply the noise the layers hold
    got["forward_fused"] = net.forward_fused(x, taus=taus)
    res = net.quantiles(x, taus=taus)
    got["quantiles"] = (res.quantiles, res.taus)
    monkeypatch.setattr(torch, "rand", lambda *shape, **kw: taus.reshape(shape))
    got["forward"] = net(x, N)
    monkeypatch.undo()
    for name, (q, t) in got.items():
        assert tuple(q.shape) == (B, N, net.action_space) and tuple(t.shape) == (B, N, 1), name
        LK.same_bits(q.detach().numpy(), got["forward"][0].detach().numpy(), "quantiles", (name, training))
        LK.same_bits(t.numpy(), taus.numpy().reshape(B, N, 1), "taus", (name, training))
    with torch.no_grad():
        mean, _ = net.forward_flat(x.view(B, -1), N, taus, noise=False)
    assert torch.equal(mean, got["forward"][0]) != training                       # the noise shows where it is applied, and only there


def test_actor_and_learner_act_alike_on_the_cpu():
    from sorrel_amd.models import IQNActor

    obs, n_frames, L, N, A, B = LC.SHAPES[0]
    learner = LC.make_model(LC.SHAPES[0], "cpu")
    local = learner.qnetwork_local
    with torch.no_grad():
        for name in ("ff_1", "advantage", "value"):
            getattr(local, name).sigma_weight.fill_(0.5)   # noise would show
            getattr(local, name).epsilon_weight.normal_()
    actor = IQNActor((obs,), A, layer_size=L, n_quantiles=N, n_frames=n_frames, seed=1)
    actor.net.load_state_dict(local.state_dict())
    nets = (actor.net, local)
    flags = [[m.training for m in net.modules()] for net in nets]
    assert flags[0] == [False] * len(flags[0]) and flags[1] == [True] * len(flags[1])
    buffers = [{k: v.clone() for k, v in net.state_dict().items()} for net in nets]
    x = torch.randn(B, obs * n_frames)
    got = []
    for model in (actor, learner):
        torch.manual_seed(7)                               # the same taus
        got.append(model.take_action(x))
    for q in got:
        assert q.shape == (B, A) and q.dtype == torch.float32 and not q.requires_grad
    LK.same_bits(got[0].numpy(), got[1].numpy(), "action values")
    assert [[m.training for m in net.modules()] for net in nets] == flags
    for net, before in zip(nets, buffers):
        assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())


def test_hooks_are_checked():
    m = LC.fill_memory(LC.make_model(LC.SHAPES[0], "cpu"))
    with pytest.raises(ValueError, match="taus="):
        m.train_step(taus=[torch.zeros(6, 5)])
    with pytest.raises(ValueError, match="noise="):
        m.train_step(noise=[torch.zeros(1)] * 6)


def test_thirty_steps_on_one_batch_lower_its_loss():
    case = LC.load_fixture()[LC.tag_of(LC.SHAPES[1])]
    args = LC.step_args(case["steps"][0], "cpu")
    m = LC.fill_memory(LC.put_state(LC.make_model(case["shape"], "cpu", LR=0.01), case["snaps"][0]))
    first = eval_loss(m, args)
    for _ in range(30):
        m.train_step(batch=args["batch"])
    last = eval_loss(m, args)
    print(first, "->", last)
    assert m.steps_done == 30 and last < first


def test_example_builds_the_learner_from_the_config():
    from sorrel_amd.examples.treasurehunt import main as TH

    cfg = TH.make_config()
    cfg["model"].update(layer_size=32, memory_size=64, batch_size=8, n_frames=2, LR=0.002, epsilon=0.25)
    factory = TH.iqn_model_factory(cfg, num_envs=8, device="cpu", seed=5)
    a, b = factory((150,), 4), factory((150,), 4)
    assert (a.layer_size, a.batch_size, a.n_frames, a.memory.capacity, a.memory.num_envs, a.epsilon) == (32, 8, 2, 64, 8, 0.25)
    assert a.optimizer.param_groups[0]["lr"] == 0.002 and a.n_quantiles == TH.IQN_DEFAULTS["n_quantiles"]
    assert a.key_seed == 5 and b.key_seed == 6
    with pytest.raises(ValueError, match="unknown model"):
        TH.make_env(cfg, 8, model="ppo")
