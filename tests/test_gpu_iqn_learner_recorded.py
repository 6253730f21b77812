"""GPU tests of the recorded learner step (``PyTorchIQN.capture_train_step``): replays are the eager steps of a twin whose optimiser also
counts on the device -- losses, parameters, target, both moments and every gradient bit for bit --, the ring may grow under a recording, an
override between replays keeps the count, moved tensors drop the recording instead of raising, a replay allocates nothing, and the
Treasurehunt example runs with a recorded turn and a recorded step in one process."""
import copy

import numpy as np
import pytest
import torch

from tests import iqn_learner_common as LC
from tests import learner_common as LK

pytestmark = pytest.mark.gpu
DEV = LK.DEV


def eager_twin(shape, rows=None, **kw):
    """The reference path: the same seed, the optimiser counting on the device before its first step, every step eager."""
    model = LC.fill_memory(LC.make_model(shape, DEV, **kw), rows=rows)
    model.optimizer.count_on_device(True)
    return model


def grads(model):
    return [p.grad.detach().cpu().numpy().copy() for p in model.qnetwork_local.parameters()]


def clock_words(model):
    torch.cuda.synchronize()
    return model._clock.tolist()


def assert_same(a, b, ctx):
    LC.same_state(LC.get_state(a), LC.get_state(b), ctx=ctx)
    for k, (x, y) in enumerate(zip(grads(a), grads(b))):
        LK.same_bits(x, y, f"grad {k}", ctx)
    assert a.steps_done == b.steps_done, ctx


@pytest.mark.parametrize("shape", LC.SHAPES, ids=LC.tag_of)
def test_recorded_steps_are_the_eager_steps(built, shape):
    a = LC.fill_memory(LC.make_model(shape, DEV))
    rec = a.capture_train_step(warmup=2)
    assert rec is a._recorded and rec.graph is not None and a.optimizer.device_step and a.steps_done == 2
    b = eager_twin(shape)
    want = [float(b.train_step()) for _ in range(2)]
    assert float(a._loss32) == want[1]                                      # the warm-up steps were real ones
    assert_same(a, b, "after the warm-up")
    got = []
    for k in range(3):
        loss = a.train_step()
        got.append(float(loss))
        want.append(float(b.train_step()))
        assert loss.data_ptr() == a._loss32.data_ptr() and loss.dtype == torch.float32 and loss.dim() == 0
    assert got == want[2:] and len(set(want)) == 5 and all(np.isfinite(want)), (got, want)
    assert rec.replays == 3 and a._recorded is rec
    assert_same(a, b, "after three replays")
    assert a.steps_done == 5 and clock_words(a)[0] == 5 and clock_words(a)[2:] == [0, 0]
    assert torch.equal(a._sampler.last_index, b._sampler.last_index)


def test_the_ring_grows_under_a_recording(built):
    shape = LC.SHAPES[1]                                                      # n_frames = 5
    kw = dict(batch_size=6)                                                   # the gate opens at 7 rows, where num_starts() = max(1, 7 - 5 - 1) = 1
    a = LC.fill_memory(LC.make_model(shape, DEV, **kw), rows=7)
    b = eager_twin(shape, rows=7, **kw)
    a.capture_train_step(warmup=1)
    at_capture = a._sampler.num_starts()
    assert at_capture == 1 and clock_words(a)[1] == 1
    b.train_step()
    assert float(a.train_step()) == float(b.train_step())
    assert int(b._sampler.last_index[:, 0].max()) == 0
    for model in (a, b):
        LC.fill_memory(model, rows=20, seed=5)
    assert a._sampler.num_starts() == 21
    for k in range(2):
        assert float(a.train_step()) == float(b.train_step()), k
        assert int(b._sampler.last_index[:, 0].max()) >= at_capture           # the eager twin draws from rows that did not exist at capture time
        assert torch.equal(a._sampler.last_index, b._sampler.last_index)
    assert a._recorded is not None and a._recorded.replays == 3
    assert clock_words(a)[:2] == [4, 21]
    assert_same(a, b, "after the ring grew")


@pytest.mark.parametrize("shape", LC.SHAPES, ids=LC.tag_of)
def test_an_override_between_replays_keeps_the_count(built, shape):
    batch = LC.step_args(LC.load_fixture()[LC.tag_of(shape)]["steps"][0], DEV)["batch"]
    a = LC.fill_memory(LC.make_model(shape, DEV))
    b = eager_twin(shape)
    rec = a.capture_train_step(warmup=1)
    b.train_step()
    for model in (a, b):
        first = float(model.train_step())
        second = float(model.train_step(batch=batch))
        third = float(model.train_step())
        model.losses = (first, second, third)
    assert a.losses == b.losses and len(set(a.losses)) == 3
    assert a._recorded is rec and rec.replays == 2
    assert_same(a, b, "replay, override, replay")
    assert a.steps_done == 4 and clock_words(a)[0] == a.steps_done


def test_moved_tensors_drop_the_recording(built, tmp_path):
    shape = LC.SHAPES[1]
    a = LC.fill_memory(LC.make_model(shape, DEV))
    b = eager_twin(shape)
    a.capture_train_step(warmup=2)
    a.train_step()
    for _ in range(3):
        b.train_step()
    assert_same(a, b, "before anything moved")
    for model in (a, b):                                                      # new moment tensors
        model.optimizer.load_state_dict(copy.deepcopy(model.optimizer.state_dict()))
    assert a._recorded is not None
    assert float(a.train_step()) == float(b.train_step())
    assert a._recorded is None                                                # dropped, not raised
    assert_same(a, b, "after load_state_dict")
    a.capture_train_step(warmup=1)                                            # a later capture records again
    b.train_step()
    assert float(a.train_step()) == float(b.train_step())
    assert a._recorded is not None and a._recorded.replays == 1
    assert_same(a, b, "recorded again")
    path = str(tmp_path / "twin.pt")
    b.save(path)
    for model in (a, b):
        model.load(path)
    assert float(a.train_step()) == float(b.train_step())
    assert a._recorded is None
    assert_same(a, b, "after load()")
    assert a.steps_done == 7


def test_release_returns_to_the_eager_path(built):
    shape = LC.SHAPES[0]
    a = LC.fill_memory(LC.make_model(shape, DEV))
    b = eager_twin(shape)
    a.capture_train_step(warmup=1)
    a.train_step()
    a.release_train_step()
    assert a._recorded is None and a.optimizer.device_step
    losses = [float(a.train_step()) for _ in range(2)]
    assert losses == [float(b.train_step()) for _ in range(4)][2:]
    assert_same(a, b, "after release")


def test_replays_allocate_nothing(built):
    a = LC.fill_memory(LC.make_model(LC.SHAPES[1], DEV))
    a.capture_train_step(warmup=2)
    kept = [a.train_step() for _ in range(2)]
    torch.cuda.synchronize()
    stats = torch.cuda.memory_stats()
    if "allocation.all.allocated" not in stats:
        pytest.skip("torch.cuda.memory_stats() has no allocation.all.allocated counter")
    before = stats["allocation.all.allocated"]
    for _ in range(3):
        kept.append(a.train_step())
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    assert len({t.data_ptr() for t in kept}) == 1 and a.steps_done == 7 and a._recorded.replays == 5


def test_updates_per_call_recorded_equals_single_replays(built):
    shape = LC.SHAPES[1]
    a = LC.fill_memory(LC.make_model(shape, DEV))
    b = LC.fill_memory(LC.make_model(shape, DEV))
    for model in (a, b):
        model.capture_train_step(warmup=1)
    a.updates_per_call = 4
    last = float(a.train_step())
    singles = [float(b.train_step()) for _ in range(4)]
    assert last == singles[-1] and len(set(singles)) == 4
    assert a._recorded.replays == b._recorded.replays == 4 and a.steps_done == 5
    assert_same(a, b, "four updates in one call")
    a.train_step(batch=LC.step_args(LC.load_fixture()[LC.tag_of(shape)]["steps"][0], DEV)["batch"])
    assert a.steps_done == 6                                                  # with overrides: exactly one step


def test_treasurehunt_example_with_a_recorded_turn_and_a_recorded_step(built):
    from sorrel_amd.examples.treasurehunt import main as TH

    cfg = TH.make_config(height=9, width=9, num_agents=2, radius=2, spawn_prob=0.05, epochs=2, max_turns=12)      # three epochs of 12 turns
    cfg["model"].update(layer_size=32, memory_size=64, batch_size=8, capture_train_step=True, updates_per_call=2)
    cfg["experiment"]["capture_turns"] = True
    env = TH.make_env(cfg, 8, model="iqn", device=DEV, seed=3)
    start = [[p.detach().clone() for p in agent.model.qnetwork_local.parameters()] for agent in env.agents]
    history = env.run_experiment(logging=False)
    assert len(history) == 3 and env.turn == 12
    assert env._captured is not None, getattr(env, "capture_error", None)
    assert np.isfinite(history[-1]["loss"]) and history[-1]["loss"] != 0.0
    for agent, before in zip(env.agents, start):
        model = agent.model
        assert model.capture_error is None and model._recorded is not None, model.capture_error
        assert model.steps_done == 3 * 2                                      # every epoch of this run is gated (12 turns x 8 envs fill the ring past 8)
        assert model._recorded.replays == 4                                   # the first call's two updates were the warm-up
        assert clock_words(model)[0] == model.steps_done
        assert any(not torch.equal(p, q) for p, q in zip(model.qnetwork_local.parameters(), before))
        assert all(bool(torch.isfinite(p).all()) for p in model.qnetwork_local.parameters())
    env.raise_on_status()
