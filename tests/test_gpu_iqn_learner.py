"""GPU tests of the IQN learner's device path (``PyTorchIQN.train_step`` on a HIP device: ``sgw_sample``, ``sgw_noisy_weights``, three
``sgw_iqn_forward``, ``sgw_iqn_loss``, ``sgw_iqn_backward``, ``sgw_noisy_weights`` backwards, ``sgw_adam_step``): the composition leaves the bits
of the hand-written step of ``sorrel_amd/losses.py``'s docstring, the reference's recorded steps land within the cap, a step allocates
nothing, the learner learns, and the Treasurehunt example runs with it, eagerly and recorded."""
import copy

import numpy as np
import pytest
import torch

from tests import iqn_learner_common as LC
from tests import learner_common as LK
from tests.test_iqn_learner_cpu import eval_loss

pytestmark = pytest.mark.gpu
DEV = LK.DEV
REFERENCE_SHAPE = (175, 5, 250, 12, 4, 64)            # in_features 875, layer 250, 12 quantiles, 4 actions, a batch of 64


class pinned_noise:
    """While open, ``Tensor.normal_`` leaves a tensor as it is: a noisy layer applies the epsilon it holds."""

    def __enter__(self):
        self.real = torch.Tensor.normal_
        torch.Tensor.normal_ = lambda t, *a, **k: t

    def __exit__(self, *exc):
        torch.Tensor.normal_ = self.real


def _set_eps(net, six):
    for k, name in enumerate(("ff_1", "advantage", "value")):
        layer = getattr(net, name)
        layer.epsilon_weight.copy_(six[2 * k])
        layer.epsilon_bias.copy_(six[2 * k + 1])


def _hand_written_step(local, target, optimizer, args, discount):
    """The step of ``losses.py``'s docstring from public calls, with the given batch, taus and noise."""
    from sorrel_amd.losses import iqn_loss

    states, actions, rewards, next_states, dones, valid = args["batch"]
    t, noise = args["taus"], args["noise"]
    with pinned_noise():
        _set_eps(local, noise[0:6])
        q_next_local = local.quantiles(next_states, taus=t[0]).quantiles
        _set_eps(target, noise[6:12])
        q_next_target = target.quantiles(next_states, taus=t[1]).quantiles
        _set_eps(local, noise[12:18])
        q_expected, taus = local.forward_fused(states, taus=t[2])
    loss = iqn_loss(q_expected, taus, q_next_local, q_next_target, actions, rewards, dones, valid, discount)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    optimizer.step()
    return loss


def _drawn_args(shape, seed):
    obs, n_frames, L, N, A, B = shape
    g = torch.Generator().manual_seed(seed)
    D = obs * n_frames
    batch = (torch.randn((B, D), generator=g), torch.randint(0, A, (B, 1), generator=g), torch.randn((B, 1), generator=g),
             torch.randn((B, D), generator=g), (torch.rand((B, 1), generator=g) < 0.2).float(), (torch.rand((B, 1), generator=g) < 0.8).float())
    taus = [torch.rand((B, N), generator=g) for _ in range(3)]
    sizes = [(L, L), (L,), (A, L), (A,), (1, L), (1,)]
    noise = [torch.randn(s, generator=g) for _ in range(3) for s in sizes]
    return dict(batch=tuple(x.to(DEV) for x in batch), taus=[x.to(DEV) for x in taus], noise=[x.to(DEV) for x in noise])


def _optimizer_state(optimizer, net):
    names = [n for n, _ in net.named_parameters()]
    st = optimizer.state_dict()["state"]
    return {n: (st[i]["exp_avg"].cpu().numpy(), st[i]["exp_avg_sq"].cpu().numpy(), int(st[i]["step"])) for i, n in enumerate(names)}


@pytest.mark.parametrize("shape", LC.SHAPES + (REFERENCE_SHAPE,), ids=LC.tag_of)
def test_composition_leaves_the_bits_of_the_hand_written_step(built, shape):
    from sorrel_amd.optim import FusedAdam

    model = LC.make_model(shape, DEV)
    fixture = LC.load_fixture().get(LC.tag_of(shape))
    if fixture is not None:
        LC.put_state(model, fixture["snaps"][1])                                   # moments and a step count from the reference's run
        start = fixture["snaps"][1]
    LC.fill_memory(model, rows=model.batch_size + 1)
    local, target = copy.deepcopy(model.qnetwork_local), copy.deepcopy(model.qnetwork_target)
    optimizer = FusedAdam(local.parameters(), lr=LC.HYPER["LR"], max_grad_norm=1, target_params=target.parameters(), tau=LC.HYPER["TAU"])
    if fixture is not None:
        optimizer.load_state_dict(copy.deepcopy(model.optimizer.state_dict()))
    for k in range(2):
        args = LC.step_args(fixture["steps"][k], DEV) if fixture is not None else _drawn_args(shape, 100 + k)
        loss = model.train_step(**args)
        assert torch.is_tensor(loss) and loss.dtype == torch.float32 and loss.shape == () and loss.device.type == "cuda"
        want = _hand_written_step(local, target, optimizer, args, LC.HYPER["GAMMA"] ** LC.HYPER["n_step"])
        ctx = (LC.tag_of(shape), k)
        LK.same_bits(loss.cpu().numpy(), want.detach().cpu().numpy().astype(np.float32), "loss", ctx)
        for part, mine, theirs in (("local", model.qnetwork_local, local), ("target", model.qnetwork_target, target)):
            for (name, p), (_, q) in zip(mine.named_parameters(), theirs.named_parameters()):
                LK.same_bits(p.detach().cpu().numpy(), q.detach().cpu().numpy(), f"{part}/{name}", ctx)
        got, ref = _optimizer_state(model.optimizer, model.qnetwork_local), _optimizer_state(optimizer, local)
        for name in ref:
            LK.same_bits(got[name][0], ref[name][0], f"exp_avg/{name}", ctx)
            LK.same_bits(got[name][1], ref[name][1], f"exp_avg_sq/{name}", ctx)
            assert got[name][2] == ref[name][2] == (k + 1 + (start["step"] if fixture is not None else 0)), ctx
        for (name, p), (_, q) in zip(model.qnetwork_local.named_parameters(), local.named_parameters()):    # the gradients themselves
            LK.same_bits(p.grad.cpu().numpy(), q.grad.cpu().numpy(), f"grad/{name}", ctx)
    assert model.steps_done == 2 + (start["step"] if fixture is not None else 0)


@pytest.mark.parametrize("tag, k", [(LC.tag_of(s), k) for s in LC.SHAPES for k in range(LC.STEPS)])
def test_recorded_steps_of_the_reference_within_the_cap(built, tag, k):
    case = LC.load_fixture()[tag]
    rec = case["steps"][k]
    model = LC.fill_memory(LC.put_state(LC.make_model(case["shape"], DEV), case["snaps"][k]), rows=case["shape"][5] + 1)
    loss = model.train_step(**LC.step_args(rec, DEV))
    print(tag, k, "loss", float(loss), "reference", float(rec["loss"]))
    assert abs(float(loss) - float(rec["loss"])) <= 1e-5 * max(1.0, abs(float(rec["loss"])))
    worst = 0.0
    for part, net in (("local", model.qnetwork_local), ("target", model.qnetwork_target)):
        sd = net.state_dict()
        for name in case["param_names"]:
            p64 = rec["after64"][part][name]
            d_ref, d_r = rec["d_ref"][f"{part}/{name}"], LC.distance(sd[name].cpu().numpy(), p64)
            limit = LC.cap(d_ref, p64)
            worst = max(worst, d_r / limit)
            print(f"| {tag} | {k} | {part}/{name} | {d_ref:.3e} | {d_r:.3e} | {limit:.3e} |")
            assert d_r <= limit, (tag, k, part, name, d_r, d_ref, limit)
    print(tag, k, "worst d_r / cap =", worst)
    got = LC.get_state(model)
    assert got["step"] == k + 1
    LK.same_bits(got["local"]["ff_1.epsilon_weight"], case["snaps"][k]["local"]["ff_1.epsilon_weight"], "the module's epsilon buffers are not used")


def test_gate_on_the_device(built):
    model = LC.fill_memory(LC.make_model(LC.SHAPES[0], DEV), rows=LC.SHAPES[0][5])
    before = LC.get_state(model)
    loss = model.train_step()
    assert torch.is_tensor(loss) and loss.dtype == torch.float32 and float(loss) == 0.0 and model.steps_done == 0
    LC.same_state(LC.get_state(model), before)
    LC.fill_memory(model, rows=8)
    again = model.train_step()
    assert again.data_ptr() == loss.data_ptr() and float(again) != 0.0 and np.isfinite(float(again)) and model.steps_done == 1


def test_drawn_steps_are_reproducible_from_their_number_and_allocate_nothing(built):
    shape = LC.SHAPES[1]

    def run(steps):
        model = LC.fill_memory(LC.make_model(shape, DEV))
        losses = [model.train_step().clone() for _ in range(steps)]
        return model, losses

    a, la = run(2)                                                                  # two warm-up steps
    torch.cuda.synchronize()
    stats = torch.cuda.memory_stats()
    if "allocation.all.allocated" not in stats:
        pytest.skip("torch.cuda.memory_stats() has no allocation.all.allocated counter")
    before = stats["allocation.all.allocated"]
    kept = []
    for _ in range(3):
        kept.append(a.train_step())
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    assert kept[0].data_ptr() == kept[2].data_ptr() and a.steps_done == 5
    b, lb = run(5)                                                                  # the same seed: the same batches, taus and noise
    assert [float(x) for x in la] == [float(x) for x in lb[:2]] and float(kept[2]) == float(lb[4])
    LC.same_state(LC.get_state(a), LC.get_state(b))
    assert len({float(x) for x in lb}) == 5                                        # and every step draws anew


def test_thirty_steps_on_one_batch_lower_its_loss(built):
    case = LC.load_fixture()[LC.tag_of(LC.SHAPES[1])]
    args = LC.step_args(case["steps"][0], DEV)
    model = LC.fill_memory(LC.put_state(LC.make_model(case["shape"], DEV, LR=0.01), case["snaps"][0]), rows=case["shape"][5] + 1)
    first = eval_loss(model, args)
    for _ in range(30):
        model.train_step(batch=args["batch"])
    last = eval_loss(model, args)
    print(first, "->", last)
    assert model.steps_done == 30 and np.isfinite(last) and last < first


def test_take_action_is_the_mean_weights_forward(built):
    model = LC.make_model(LC.SHAPES[1], DEV)
    net = model.qnetwork_local
    with torch.no_grad():
        for name in ("ff_1", "advantage", "value"):
            getattr(net, name).sigma_weight.fill_(0.5)
    x = torch.randn((33, 35), device=DEV)
    q = model.take_action(x).clone()
    assert net.training and q.shape == (33, 5) and q.dtype == torch.float32
    net.eval()
    want = net.quantiles(x, key={"turn": net._calls}).qvalues
    net.train()
    assert torch.equal(q, want)


def test_bound_actor_and_learner_act_alike_eagerly_and_in_a_recorded_turn(built):
    from sorrel_amd.models import IQNActor, PyTorchIQN
    from tests.gpu_common import make_env

    E, A, T = 2, 2, 2

    def build(learner):
        made = []

        def factory(input_size, action_space):
            seed = 100 + len(made)
            if learner:
                made.append(PyTorchIQN(input_size, action_space, 33, 0.0, DEV, seed, n_frames=1, n_quantiles=5, batch_size=4, memory_size=8, num_envs=E))
            else:
                made.append(IQNActor(input_size, action_space, layer_size=33, n_quantiles=5, seed=seed, memory_size=8, num_envs=E, device=DEV))
            return made[-1]

        env = make_env(8, 8, A, 2, E, p=0.05, seed=23, model_factory=factory)
        for a, agent in enumerate(env.agents):
            agent.model.bind(env, a)
        return env

    acting, learning = build(False), build(True)
    for a in range(A):
        local = learning.agents[a].model.qnetwork_local
        with torch.no_grad():
            for name in ("ff_1", "advantage", "value"):
                getattr(local, name).sigma_weight.fill_(0.5)                       # noise would show
                getattr(local, name).epsilon_weight.normal_()
        acting.agents[a].model.net.load_state_dict(local.state_dict())
        assert local.training and not acting.agents[a].model.net.training
    # eagerly: both bound to the same environment and slot, so both key their taus alike
    actor, learner = acting.agents[1].model, learning.agents[1].model
    learner.bind(acting, 1)
    x = torch.randn((E, actor.net.head1.in_features), device=DEV)
    qa, ql = actor.take_action(x).clone(), learner.take_action(x).clone()
    assert qa.shape == (E, actor.net.action_space) and qa.dtype == torch.float32
    assert torch.equal(actor._out.taus, learner._out.taus) and torch.equal(qa, ql)
    learner.bind(learning, 1)
    # recorded: the same world twice, one played by the actors and one by the learners; the device keys a replayed turn's taus
    caps = [env.capture_turn(warmup=1, force=True) for env in (acting, learning)]
    assert caps[0] is not None and caps[1] is not None, (acting.capture_error, learning.capture_error)
    seen = []
    for t in range(T):
        acting.take_turn()
        learning.take_turn()
        torch.cuda.synchronize()
        for a in range(A):
            oa, ol = acting.agents[a].model._out, learning.agents[a].model._out
            assert torch.equal(oa.taus, ol.taus) and torch.equal(oa.qvalues, ol.qvalues), (t, a)
        seen.append(acting.agents[0].model._out.taus.clone())
        assert torch.equal(acting.actions, learning.actions), t
    assert caps[0].turns_replayed == T and caps[1].turns_replayed == T and not torch.equal(seen[0], seen[1])
    assert all(agent.model.qnetwork_local.training for agent in learning.agents)
    acting.raise_on_status()
    learning.raise_on_status()


def _example(capture):
    from sorrel_amd.examples.treasurehunt import main as TH

    cfg = TH.make_config(height=9, width=9, num_agents=2, radius=2, spawn_prob=0.05, epochs=2, max_turns=12)
    cfg["model"].update(layer_size=32, memory_size=64, batch_size=8)
    cfg["experiment"]["capture_turns"] = capture
    env = TH.make_env(cfg, 8, model="iqn", device=DEV, seed=3)
    start = [[p.detach().clone() for p in agent.model.qnetwork_local.parameters()] for agent in env.agents]
    history = env.run_experiment(logging=False)
    return env, start, history


def test_treasurehunt_example_learns_eagerly_and_recorded(built):
    from sorrel_amd.models import PyTorchIQN

    env, start, history = _example(False)
    assert len(history) == 3 and env.turn == 12
    assert all(isinstance(agent.model, PyTorchIQN) for agent in env.agents)
    assert np.isfinite(history[-1]["loss"]) and history[-1]["loss"] != 0.0
    for agent, before in zip(env.agents, start):
        assert agent.model.steps_done == 3
        assert any(not torch.equal(p, q) for p, q in zip(agent.model.qnetwork_local.parameters(), before))
        assert all(bool(torch.isfinite(p).all()) for p in agent.model.qnetwork_local.parameters())
    env.raise_on_status()
    rec, _, rec_history = _example(True)
    assert rec._captured is not None, getattr(rec, "capture_error", None)
    assert len(rec_history) == 3 and rec.turn == env.turn == 12
    assert [a.model.memory.size for a in rec.agents] == [a.model.memory.size for a in env.agents]
    assert np.isfinite(rec_history[-1]["loss"]) and rec_history[-1]["loss"] != 0.0
    rec.raise_on_status()
