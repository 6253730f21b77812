"""TEST INFRASTRUCTURE ONLY -- generate ``tests/golden/iowa/iowa_*.npz`` from the reference's Iowa Gambling Task.

Needs the reference checkout (``oracle/ref_loader.py``).  Usage::

    PYTHONDONTWRITEBYTECODE=1 python tools/make_iowa_golden.py

What runs is the reference's own ``Environment.take_turn`` -> entity sweep -> ``GamblingAgent.transition`` / ``act`` ->
``Gridworld.move`` (sorrel/environment.py:81-93, sorrel/examples/iowa/agents.py:47-60) on the reference's own ``GamblingWorld``,
``Wall``, ``Sand`` and ``GamblingAgent``.  Supplied here, as a user of the plugin API would: a ``Deck`` and an ``EmptyEntity`` whose
random calls come from the counter generator (the way ``oracle/make_golden.py``'s ``CounterEmpty`` does it), a counter-driven model,
``setup_agents`` / ``populate_environment``.  The plugin ``Deck`` keeps the reference's ``draw()`` arithmetic: only the number
``np.random.random()`` returns inside it is replaced.

Each fixture stores per-turn grid, positions, windows, actions, rewards, ``world.total_reward`` and the deck kind every agent stepped on
(from ``GamblingAgent.encounters``).  Data only: no reference source text is stored.  The generator asserts what makes equality mean
something -- every deck stepped on with both outcomes, at least one deck stepped on in the turn it was spawned -- and that
``tests/iowa_common.expected_run`` reproduces every array."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import gridstep_oracle as O  # noqa: E402
from oracle import make_golden as MG  # noqa: E402
from oracle.make_golden import Ctx  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import iowa_common as I  # noqa: E402

# (name, height, width, agents, radius, spawn_prob, seed, envs, turns)
FIXTURES = (
    ("iowa_9x9_dense", 9, 9, 2, 2, 0.10, 11, 4, 40),
    ("iowa_20x20_default", 20, 20, 2, 2, 0.01, 5, 4, 100),
    ("iowa_12x10_three_agents", 12, 10, 3, 2, 0.08, 7, 3, 40),
)
LOSS_PROB = {"a": 0.5, "b": 0.1, "c": 0.5, "d": 0.1}     # the constants Deck.draw compares p_loss with


def run_reference_iowa(R, ws, env_ids, turns, epoch=0):
    import sorrel.examples.iowa.agents as iowa_agents
    import sorrel.examples.iowa.entities as iowa_entities
    import sorrel.examples.iowa.world as iowa_world

    _, CounterModel, _ = MG.build_plugins(R)
    Environment = R["environment"].Environment
    OneHot = R["observation_spec"].OneHotObservationSpec
    ActionSpec = R["action_spec"].ActionSpec
    Agent = R["agents"].Agent
    spec = H.oracle_spec(ws)

    class CounterDeck(iowa_entities.Deck):
        """The reference's Deck; the one random number of ``draw()`` comes from stream 8 of the counter generator, keyed by the deck's
        cell and the turn, under the threshold convention (u32 < floor(p * 2^32)): the number handed to ``draw()`` is 0.0 for a loss
        and 1.0 otherwise, and ``draw()`` itself does the arithmetic."""

        swept = False

        def transition(self, world):
            y, x, z = self.location
            u = int(O.rng_u32(Ctx.seed, Ctx.env, Ctx.epoch, Ctx.turn, I.STREAM_VALUE, int(O.cell_index(spec, y, x, z))))
            number = 0.0 if u < O.prob_threshold(LOSS_PROB[self.name]) else 1.0
            saved = np.random.random
            np.random.random = lambda: number
            try:
                super().transition(world)
            finally:
                np.random.random = saved
            self.swept = True

    class CounterEmpty(iowa_entities.EmptyEntity):
        def __init__(self):
            super().__init__()
            self.kind = "EmptyEntity"         # (a subclass's kind is its own class name by default)

        def transition(self, world):
            y, x, z = self.location
            idx = int(O.cell_index(spec, y, x, z))
            if int(O.rng_u32(Ctx.seed, Ctx.env, Ctx.epoch, Ctx.turn, O.STREAM_SPAWN, idx)) < O.prob_threshold(world.spawn_prob):
                k = int(O.categorical(O.rng_u32(Ctx.seed, Ctx.env, Ctx.epoch, Ctx.turn, O.STREAM_SPAWN_KIND, idx), 4))
                world.add(self.location, CounterDeck("abcd"[k]))

    class HarnessEnv(Environment):
        def setup_agents(self):
            self.agents = []
            for slot in range(ws.num_agents):
                ospec = OneHot(list(I.ENTITY_LIST), full_view=False, vision_radius=ws.vision_radius)
                ospec.override_input_size((int(np.prod(ospec.input_size)),))
                aspec = ActionSpec(["up", "down", "left", "right"])
                model = CounterModel(ospec.input_size, aspec.n_actions, memory_size=turns + 1, slot=slot)
                self.agents.append(iowa_agents.GamblingAgent(observation_spec=ospec, action_spec=aspec, model=model))

        def populate_environment(self):
            Hh, Ww = self.world.height, self.world.width
            for index in np.ndindex(self.world.map.shape):
                y, x, z = index
                if y in [0, Hh - 1] or x in [0, Ww - 1]:
                    self.world.add(index, iowa_entities.Wall())
                elif z == 0:
                    self.world.add(index, iowa_entities.Sand())
            for (y, x), agent in zip(O.place_agents(spec, Ctx.env, Ctx.epoch), self.agents):
                self.world.add((int(y), int(x), 1), agent)

    def type_ids(world):
        Hh, Ww, L = world.map.shape
        g = np.zeros((L, Hh, Ww), dtype=np.uint8)
        for (y, x, z), e in np.ndenumerate(world.map):
            if isinstance(e, Agent):
                t = I.AGENT_T
            elif type(e) is iowa_entities.Sand:
                t = 0
            elif type(e) is CounterEmpty:
                t = 1
            elif type(e) is iowa_entities.Wall:
                t = 2
            elif type(e) is CounterDeck:
                t = (I.DRAWN0 if e.swept else I.FRESH0) + "abcd".index(e.name)
                assert e.swept or e.value == 0
            else:
                raise RuntimeError(f"unmapped entity {e!r}")
            assert tuple(e.location) == (y, x, z), "entity.location out of sync with the map"
            g[z, y, x] = t
        return g

    E, A, C, V = len(env_ids), ws.num_agents, ws.num_channels, ws.window
    out = dict(
        grid0=np.zeros((E, 2, ws.height, ws.width), np.uint8), pos0=np.zeros((E, A, 2), np.uint8),
        obs=np.zeros((turns, E, A, C, V, V), np.float32), actions=np.zeros((turns, E, A), np.uint8),
        rewards=np.zeros((turns, E, A), np.float32), total_reward=np.zeros((turns, E), np.float64),
        grid=np.zeros((turns, E, 2, ws.height, ws.width), np.uint8), pos=np.zeros((turns, E, A, 2), np.uint8),
        target_kinds=np.full((turns, E, A), -1, np.int8),
    )
    cfg = {"world": {"height": ws.height, "width": ws.width, "spawn_prob": ws.spawn_prob[1]},
           "experiment": {"epochs": 1, "max_turns": turns, "record_period": 1}}
    for n, env_id in enumerate(env_ids):
        Ctx.seed, Ctx.env, Ctx.epoch, Ctx.turn, Ctx.spec, Ctx.scripted = ws.seed, int(env_id), epoch, 0, spec, None
        env = HarnessEnv(iowa_world.GamblingWorld(config=cfg, default_entity=CounterEmpty()), cfg)
        out["grid0"][n] = type_ids(env.world)
        out["pos0"][n] = [a.location[:2] for a in env.agents]
        for t in range(turns):
            Ctx.turn = env.turn + 1
            seen = [dict(a.encounters) for a in env.agents]
            env.take_turn()                             # <- the reference's hot path
            for a, agent in enumerate(env.agents):
                mem = agent.model.memory
                out["obs"][t, n, a] = mem.states[t].reshape(C, V, V)
                out["actions"][t, n, a] = mem.actions[t]
                out["rewards"][t, n, a] = mem.rewards[t]
                out["pos"][t, n, a] = agent.location[:2]
                hit = [k for k in I.DECK_KINDS if agent.encounters[k] != seen[a][k]]
                assert len(hit) <= 1
                if hit:
                    out["target_kinds"][t, n, a] = I.DECK_KINDS.index(hit[0])
            out["total_reward"][t, n] = env.world.total_reward
            out["grid"][t, n] = type_ids(env.world)
    return out


def check_coverage(name, ref, mine):
    cov = I.coverage(mine)
    assert cov["fresh"] >= 1, f"{name}: no deck was stepped on in the turn it was spawned"
    for kind, (plain, loss) in cov["pairs"].items():
        assert plain >= 1 and loss >= 1, f"{name}: {kind} was not stepped on with both outcomes ({plain}, {loss})"
    assert int((ref["target_kinds"] >= 0).sum()) == cov["fresh"] + cov["drawn"]
    return cov


def main():
    R = MG._import_reference()
    os.makedirs(I.IOWA_DIR, exist_ok=True)
    for name, h, w, agents, radius, sp, seed, envs, turns in FIXTURES:
        ws = I.iowa_spec(h, w, agents, radius, sp, seed)
        ref = run_reference_iowa(R, ws, list(range(envs)), turns)
        mine = I.expected_run(ws, envs, turns, actions=ref["actions"])
        for key in ("grid0", "pos0", "grid", "pos", "obs", "actions", "rewards", "total_reward"):
            assert np.array_equal(ref[key], mine[key]), f"{name}: the checker's {key} differs from the reference's"
        assert np.array_equal(ref["target_kinds"], I.fold_kinds(mine["target_types"])), f"{name}: target kinds differ"
        free = I.expected_run(ws, envs, turns)          # the engine's own action draws are the counter model's
        assert np.array_equal(free["actions"], ref["actions"])
        cov = check_coverage(name, ref, mine)
        path = os.path.join(I.IOWA_DIR, name + ".npz")
        np.savez_compressed(path, spec_json=np.array(I.spec_to_json(ws)), num_envs=np.array(envs), turns=np.array(turns), **ref)
        print(f"{name}: {os.path.getsize(path) >> 10} KiB, fresh hits {cov['fresh']}, drawn hits {cov['drawn']}, pairs {cov['pairs']}")


if __name__ == "__main__":
    main()
