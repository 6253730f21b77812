"""Run batched Treasurehunt rollouts: ``python -m sorrel_amd.examples.treasurehunt.main [--model iqn]``.

The default agents act at random (``RandomModel``: the whole epoch is one engine call).  ``--model iqn`` gives every agent a
``sorrel_amd.models.PyTorchIQN`` built from ``config.model.*`` with the reference's keys (``sorrel/examples/treasurehunt/env.py:80-99``): the
agents act through the network, fill its replay ring and learn after every epoch.  ``--capture-train`` records the learner's step as a graph
at its first update (``config.model.capture_train_step``); ``config.model.updates_per_call`` makes several updates per epoch (default 1, the
reference's)."""
import sys

from sorrel_amd.examples.treasurehunt.entities import EmptyEntity
from sorrel_amd.examples.treasurehunt.env import TreasurehuntEnv
from sorrel_amd.examples.treasurehunt.world import TreasurehuntWorld

#: ``config.model`` keys ``iqn_model_factory`` hands to ``PyTorchIQN`` (the reference's), and the reference example's values
IQN_DEFAULTS = dict(layer_size=250, epsilon=0.6, n_frames=5, n_step=3, sync_freq=200, model_update_freq=4, batch_size=64, memory_size=1024,
                    LR=0.00025, TAU=0.001, GAMMA=0.99, n_quantiles=12)


def make_config(height=21, width=21, num_agents=2, radius=2, spawn_prob=0.005, epochs=2, max_turns=100):
    return {
        "experiment": {"epochs": epochs, "max_turns": max_turns, "record_period": 50},
        "model": {"agent_vision_radius": radius, "num_agents": num_agents},
        "world": {"height": height, "width": width, "gem_value": 10, "food_value": 5, "bone_value": -10,
                  "spawn_prob": spawn_prob},
    }


def iqn_model_factory(config, num_envs, device=None, seed=0):
    """A ``model_factory`` for ``TreasurehuntEnv``: every agent gets its own ``PyTorchIQN`` from ``config["model"]`` (``IQN_DEFAULTS`` for
    the keys it leaves out), with a replay ring over ``num_envs`` envs; agent ``k``'s seed is ``seed + k``.  ``updates_per_call`` (default 1) and
    ``capture_train_step`` (default False: the model records its step at its first gated ``train_step``) are this package's keys."""
    from sorrel_amd.models import PyTorchIQN

    model = config["model"]
    args = {key: model[key] if key in model else default for key, default in IQN_DEFAULTS.items()}
    made = []

    def factory(input_size, action_space):
        made.append(PyTorchIQN(input_size, action_space, device=device, seed=seed + len(made), num_envs=num_envs, **args))
        made[-1].updates_per_call = int(model.get("updates_per_call", 1))
        made[-1].capture_lazily = bool(model.get("capture_train_step", False))
        return made[-1]

    return factory


def make_env(config, num_envs, model="random", device=None, seed=0):
    """The example's environment: ``model`` is ``"random"`` or ``"iqn"``."""
    if model not in ("random", "iqn"):
        raise ValueError(f"unknown model {model!r}: random or iqn")
    world = TreasurehuntWorld(config=config, default_entity=EmptyEntity(), num_envs=num_envs, **({} if device is None else {"device": device}))
    if model == "random":
        return TreasurehuntEnv(world, config)
    env = TreasurehuntEnv(world, config, model_factory=iqn_model_factory(config, num_envs, device=world.device, seed=seed))
    for slot, agent in enumerate(env.agents):
        agent.model.bind(env, slot)
    return env


if __name__ == "__main__":
    argv = sys.argv[1:]
    kind = argv[argv.index("--model") + 1] if "--model" in argv else "random"
    config = make_config()
    config["model"]["capture_train_step"] = "--capture-train" in argv
    env = make_env(config, 4096 if kind == "random" else 256, kind)
    for epoch, m in enumerate(env.run_experiment()):
        print(f"epoch {epoch}: mean total_reward over {int(m['envs'])} envs = {m['mean_total_reward']:.3f}" +
              (f", loss = {m['loss']:.5f}" if kind == "iqn" else ""))
