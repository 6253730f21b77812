"""Run batched Iowa Gambling Task rollouts: ``python -m sorrel_amd.examples.iowa.main``."""
from sorrel_amd.examples.iowa.entities import EmptyEntity
from sorrel_amd.examples.iowa.env import GamblingEnv
from sorrel_amd.examples.iowa.world import GamblingWorld


def make_config(height=20, width=20, num_agents=2, radius=2, spawn_prob=0.01, epochs=2, max_turns=100):
    """The reference's shape (``iowa/main.py:13-35``): 20x20x2, two agents, radius 2, 100 turns per epoch."""
    return {
        "experiment": {"epochs": epochs, "max_turns": max_turns, "record_period": 50},
        "model": {"agent_vision_radius": radius, "num_agents": num_agents},
        "world": {"height": height, "width": width, "spawn_prob": spawn_prob},
    }


if __name__ == "__main__":
    config = make_config()
    world = GamblingWorld(config=config, default_entity=EmptyEntity(), num_envs=4096)
    env = GamblingEnv(world, config)
    for epoch, m in enumerate(env.run_experiment()):
        print(f"epoch {epoch}: mean total_reward over {int(m['envs'])} envs = {m['mean_total_reward']:.3f}, encounters = {m['encounters']}")
