"""Checker for worlds with drawn values (the Iowa Gambling Task), independent of the code under test.

Neither oracle knows the rule, and neither needs to.  With ``type_value[t] = t + 1`` in a copy of the spec the existing C oracle's
reward IS the target's type id (+ 1; 0 = the agent had no target: an invalid action or a cell outside the grid), and grid, positions
and windows do not depend on values at all.  ``expected_run`` plays the oracle once that way and forms, from the two value tables and
the oracle module's counter RNG (``rng_u32`` / ``prob_threshold`` / ``cell_index``, stream 8): the rewards, the float64 totals in agent
order and ``target_types``."""
from __future__ import annotations

import copy
import json
import os

import numpy as np

from tests import helpers as H
from oracle import gridstep_oracle as O
from sorrel_amd.spec import NO_BORDER, RULE_BECOME_IF, RULE_SPAWN, WorldSpec, action_deltas

STREAM_VALUE = 8
NO_TARGET = 255
IOWA_DIR = os.path.join(H.GOLDEN_DIR, "iowa")      # (a directory of its own: tests/golden/*.npz are step-loop traces every oracle test replays)
DECKS = ("a", "b", "c", "d")
DECK_KINDS = ("DeckA", "DeckB", "DeckC", "DeckD")
TYPE_NAMES = ["Sand", "EmptyEntity", "Wall"] + [f"Deck{n.upper()}:fresh" for n in DECKS] + [f"Deck{n.upper()}" for n in DECKS] + ["GamblingAgent"]
FRESH0, DRAWN0, AGENT_T = 3, 7, 11
ENTITY_LIST = ["EmptyEntity", "Wall", "Sand", "DeckA", "DeckB", "DeckC", "DeckD", "GamblingAgent"]


def deck_tables():
    """(otherwise, alt, prob) per deck, in Python floats in the reference's order of operations (sorrel/examples/iowa/entities.py:45-66):
    ``value = base``; ``value += loss`` if the loss is drawn; ``return value + 0.1``."""
    out = []
    for base, loss, prob in ((1, -2.5, 0.5), (1, -12.5, 0.1), (0.5, -0.5, 0.5), (0.5, -2.5, 0.1)):
        hit = base
        hit += loss
        out.append((base + 0.1, hit + 0.1, prob))
    return out


def iowa_spec(height=20, width=20, num_agents=2, radius=2, spawn_prob=0.01, seed=0, direct=False) -> WorldSpec:
    """The Iowa world by hand: 0 Sand, 1 EmptyEntity (spawner), 2 Wall, 3-6 fresh decks A-D (value 0; become their drawn twin on the next
    sweep), 7-10 drawn decks A-D, 11 GamblingAgent.  Walls around both layers, sand below, agents and decks on layer 1.
    ``direct``: a variant without the fresh twins -- the spawner places drawn decks, which draw from their first turn on -- for the kernel
    families that run no cross-type rules (a workgroup per env)."""
    T, C = 12, len(ENTITY_LIST)
    kind = ["Sand", "EmptyEntity", "Wall"] + list(DECK_KINDS) + list(DECK_KINDS) + ["GamblingAgent"]
    app = np.zeros((T, C))
    for t, k in enumerate(kind):
        if k != "EmptyEntity":                       # (kind "EmptyEntity" is the zero vector: observation_spec.py:168-169)
            app[t, ENTITY_LIST.index(k)] = 1.0
    tab = deck_tables()
    value = [0.0, 0.0, -1.0] + [0.0] * 4 + [o for o, _a, _p in tab] + [0.0]
    alt = [0.0] * DRAWN0 + [a for _o, a, _p in tab] + [0.0]
    prob = [0.0] * DRAWN0 + [p for _o, _a, p in tab] + [0.0]
    rule = [0, RULE_SPAWN, 0] + [RULE_BECOME_IF] * 4 + [0] * 5
    choices = [3, 4, 5, 6]
    if direct:
        rule, choices = [0, RULE_SPAWN] + [0] * 10, [7, 8, 9, 10]
    dy, dx = action_deltas(["up", "down", "left", "right"])
    return WorldSpec(
        height=height, width=width, layers=2, num_agents=num_agents, vision_radius=radius, num_channels=C, agent_layer=1,
        default_type=1, fill_type=2, action_dy=dy, action_dx=dx, agent_type=[AGENT_T] * num_agents,
        type_value=value, type_value_alt=alt, value_alt_prob=prob, type_passable=[1, 1, 0] + [1] * 8 + [0], type_rule=rule,
        spawn_prob=[0.0, spawn_prob] + [0.0] * 10, spawn_choices=[[], choices] + [[]] * 10,
        rule_layer=[0] * 3 + [-1] * 4 + [0] * 5, rule_mask=[0] * T, rule_become=[0] * 3 + [7, 8, 9, 10] + [0] * 5,
        appearance=app, seed=seed, layer_fill_type=[0, 1], layer_border_type=[2, 2], type_names=list(TYPE_NAMES))


def spec_to_json(ws: WorldSpec) -> str:
    d = {k: (np.asarray(v).tolist() if isinstance(v, np.ndarray) else v) for k, v in ws.__dict__.items()}
    return json.dumps(d)


def spec_from_json(text: str) -> WorldSpec:
    d = json.loads(text)
    d["appearance"] = np.asarray(d["appearance"], dtype=np.float64)
    return WorldSpec(**d)


def type_id_spec(ws: WorldSpec) -> WorldSpec:
    """A copy the unedited oracle can play: every type is worth its id + 1, nobody draws."""
    s = copy.copy(ws)
    s.type_value = [float(t + 1) for t in range(ws.num_types)]
    s.type_value_alt, s.value_alt_prob = [], []
    return s


def expected_run(ws: WorldSpec, num_envs: int, turns: int, epoch: int = 0, actions=None, first_env_id: int = 0, first_turn: int = 1,
                 start=None, want_obs: bool = True):
    """Play ``turns`` whole turns of ``num_envs`` envs on the C oracle and return per-turn arrays: grid, pos, obs, actions, rewards
    (float32), total_reward (float64, agent order), target_types (uint8).  ``actions``: ``[turns, E, A]`` given actions, or None for
    the engine's own draws (STREAM_ACTION).  ``start``: (grid, pos, total) to go on from, else a reset of ``epoch``."""
    E, A = int(num_envs), ws.num_agents
    orc = H.COracle(type_id_spec(ws), E, first_env_id=first_env_id)
    if start is None:
        orc.reset(epoch)
        total = np.zeros((E,), np.float64)
    else:
        orc.grid[...], orc.pos[...] = start[0], start[1]
        total = np.array(start[2], dtype=np.float64, copy=True)
    out = dict(grid0=orc.grid.copy(), pos0=orc.pos.copy(),
               grid=np.zeros((turns,) + orc.grid.shape, np.uint8), pos=np.zeros((turns, E, A, 2), np.uint8),
               obs=np.zeros((turns,) + orc.obs.shape, np.float32) if want_obs else None,
               actions=np.zeros((turns, E, A), np.uint8), rewards=np.zeros((turns, E, A), np.float32),
               total_reward=np.zeros((turns, E), np.float64), target_types=np.zeros((turns, E, A), np.uint8))
    value = np.asarray(ws.type_value, dtype=np.float64)
    alt = np.zeros(ws.num_types)
    alt[:len(ws.type_value_alt)] = ws.type_value_alt
    thr = np.zeros(ws.num_types, dtype=np.uint64)
    for t, p in enumerate(ws.value_alt_prob):
        thr[t] = O.prob_threshold(p)
    dy, dx = np.asarray(ws.action_dy), np.asarray(ws.action_dx)
    ospec = H.oracle_spec(ws)
    env_ids = first_env_id + np.arange(E)
    for k in range(turns):
        turn = first_turn + k
        before = orc.pos.astype(np.int64)                                     # an agent's cell only changes by its own act
        orc.step(epoch, turn, actions=None if actions is None else actions[k], random_actions=actions is None, write_obs=want_obs)
        act = orc.actions.astype(np.int64)
        found = orc.rewards.astype(np.int64) - 1                              # type id of the target; -1: no target
        tt = np.where(found >= 0, found, NO_TARGET).astype(np.uint8)
        ok = act < ws.num_actions
        ty = before[..., 0] + np.where(ok, dy[np.minimum(act, ws.num_actions - 1)], 0)
        tx = before[..., 1] + np.where(ok, dx[np.minimum(act, ws.num_actions - 1)], 0)
        val = np.where(found >= 0, value[np.maximum(found, 0)], 0.0)
        draws = (found >= 0) & (thr[np.maximum(found, 0)] > 0)
        for e, a in zip(*np.nonzero(draws)):
            cell = int(O.cell_index(ospec, int(ty[e, a]), int(tx[e, a]), ws.agent_layer))
            u = int(O.rng_u32(ws.seed, int(env_ids[e]), epoch, turn, STREAM_VALUE, cell))
            if u < int(thr[found[e, a]]):
                val[e, a] = alt[found[e, a]]
        for a in range(A):                                                    # world.total_reward += reward: float64, agent order
            total = total + val[:, a]
        out["grid"][k], out["pos"][k], out["actions"][k] = orc.grid, orc.pos, orc.actions
        if want_obs:
            out["obs"][k] = orc.obs
        out["rewards"][k], out["total_reward"][k], out["target_types"][k] = val.astype(np.float32), total, tt
    return out


def fold_kinds(target_types: np.ndarray) -> np.ndarray:
    """Deck kind (0-3) of each target type of ``iowa_spec``'s numbering, -1 for everything else."""
    t = target_types.astype(np.int64)
    return np.where((t >= FRESH0) & (t < AGENT_T), (t - FRESH0) % 4, -1)


def coverage(run) -> dict:
    """What a trace proves: how often a fresh deck was stepped on, and for every deck how often each outcome was drawn."""
    tt, rew = run["target_types"], run["rewards"]
    tab = deck_tables()
    fresh = int(((tt >= FRESH0) & (tt < DRAWN0)).sum())
    pairs = {}
    for d in range(4):
        m = tt == DRAWN0 + d
        pairs[DECK_KINDS[d]] = (int((m & (rew == np.float32(tab[d][0]))).sum()), int((m & (rew == np.float32(tab[d][1]))).sum()))
    return dict(fresh=fresh, drawn=int(((tt >= DRAWN0) & (tt < AGENT_T)).sum()), pairs=pairs)


def fixture_names():
    if not os.path.isdir(IOWA_DIR):
        return []
    return sorted(os.path.splitext(n)[0] for n in os.listdir(IOWA_DIR) if n.startswith("iowa_") and n.endswith(".npz"))


def load_fixture(name):
    d = np.load(os.path.join(IOWA_DIR, name + ".npz"))
    return d, spec_from_json(str(d["spec_json"]))
