"""A checker for encounter counts (``sgw_bind_encounters``) that shares nothing with the code under test.

Grid dynamics do not depend on entity values.  So for each slot s the unedited C oracle plays the world once with
``type_value[t] = 1 if slot_of_type[t] == s else 0`` and nobody drawing: the reward of an act is then exactly what that act adds to slot s
-- for plain movers (the value of the type found on the agent layer of the target) and for Cleanup agents (the values of every layer of
the target, summed) alike; an invalid action or a target outside the grid is worth 0 and counts nothing.  The worlds the GPU tests play
are defined here, so that the CPU tests can assert what makes equality on them mean something."""
import copy
import os

import numpy as np

from tests import helpers as H
from tests import iowa_common as I
from sorrel_amd import _native as N
from sorrel_amd.spec import WorldSpec

NO_SLOT = 255
FIXTURE = os.path.join(H.GOLDEN_DIR, "encounters", "cleanup_15x16.npz")

# the Cleanup worlds of oracle/make_golden.cleanup_spec: 0 EmptyEntity, 1 Sand (kind EmptyEntity), 2 Wall, 3 River, 4 Pollution, 5 AppleTree,
# 6 Apple, 7 / 8 CleanBeam fresh / aged, 9 / 10 ZapBeam fresh / aged, 11 CleanupAgent
CLEANUP_KINDS = ("EmptyEntity", "Wall", "River", "Pollution", "AppleTree", "Apple", "CleanBeam", "ZapBeam", "CleanupAgent")
CLEANUP_SLOTS = [0, 0, 1, 2, 3, 4, 5, 6, 6, 7, 7, 8]
# tests/iowa_common.iowa_spec: the four deck kinds (fresh and drawn twins share a slot) plus Wall; Sand, EmptyEntity and the agents are not counted
IOWA_KINDS = I.DECK_KINDS + ("Wall",)
IOWA_SLOTS = [NO_SLOT, NO_SLOT, 4] + [0, 1, 2, 3] * 2 + [NO_SLOT]
# Treasurehunt (tests/helpers.TH_KINDS): the two EmptyEntity types share a slot, the agents are not counted
TH_KINDS = ("EmptyEntity", "Wall", "Gem", "Bone", "Food")
TH_SLOTS = [0, 0, 1, 2, 3, 4, NO_SLOT]


def slot_value_spec(ws: WorldSpec, slot_of_type, s: int) -> WorldSpec:
    """A copy the unedited oracle can play: a type is worth 1 if it counts in slot ``s``, else 0; nobody draws."""
    c = copy.copy(ws)
    c.type_value = [1.0 if slot_of_type[t] == s else 0.0 for t in range(ws.num_types)]
    c.type_value_alt, c.value_alt_prob = [], []
    return c


def expected_counts(ws: WorldSpec, slot_of_type, num_slots: int, num_envs: int, turns: int, epoch: int = 0, actions=None, first_env_id: int = 0,
                    first_turn: int = 1, start=None, agent_dir=None, auto_reset: int = 0):
    """Per-turn increments ``inc[T, E, A, K]`` (int64) of ``turns`` whole turns, with the actions played ``[T, E, A]`` and the state after the
    last turn (grid, pos, agent_dir).  ``actions``: given ``[T, E, A]``, or None for the engine's own draws (STREAM_ACTION).  ``start``:
    ``(grid, pos)`` to go on from, else a reset of ``epoch``.  ``auto_reset``: epoch length -- the turn after it is turn 1 of ``epoch + 1``,
    from a reset (``sgw_set_auto_reset``)."""
    assert len(slot_of_type) == ws.num_types and all(s == NO_SLOT or 0 <= s < num_slots for s in slot_of_type)
    E, A, K = int(num_envs), ws.num_agents, int(num_slots)
    inc = np.zeros((turns, E, A, K), dtype=np.int64)
    played = np.zeros((turns, E, A), dtype=np.uint8)
    last = None
    for s in range(K):
        orc = H.COracle(slot_value_spec(ws, slot_of_type, s), E, first_env_id=first_env_id)
        if start is None:
            orc.reset(epoch)
        else:
            orc.grid[...], orc.pos[...] = start[0], start[1]
        if agent_dir is not None:
            orc.agent_dir[...] = agent_dir
        ep, turn = epoch, first_turn
        for k in range(turns):
            orc.step(ep, turn, actions=None if actions is None else actions[k], random_actions=actions is None, write_obs=False)   # (the status word reports the bad actions: expected)
            r = orc.rewards
            assert np.array_equal(r, np.rint(r)) and (r >= 0).all()
            inc[k, :, :, s] = r.astype(np.int64)
            if s == 0:
                played[k] = orc.actions
            else:
                assert np.array_equal(played[k], orc.actions)
            if auto_reset and turn == auto_reset:
                ep, turn = ep + 1, 1
                orc.reset(ep)
            else:
                turn += 1
        state = (orc.grid.copy(), orc.pos.copy(), orc.agent_dir.copy())
        if last is not None:                 # the dynamics do not depend on the values
            assert all(np.array_equal(x, y) for x, y in zip(last, state))
        last = state
    return dict(inc=inc, cum=np.cumsum(inc, axis=0), actions=played, grid=last[0], pos=last[1], agent_dir=last[2])


# ---------------------------------------------------------------------------------------------------------------- the reference fixture
def load_fixture():
    d = np.load(FIXTURE)
    return d, H.world_spec(H.oracle_spec_from_json(str(d["spec_json"])))


def fixture_batch(d, E=8):
    """The fixture's two envs (global ids 0 and 7) inside a batch of consecutive ids 0 .. E - 1: env 7 is the fixture's second, every other
    env starts from the first one's grid and plays its actions (under its own id's spawn draws)."""
    ids = [int(i) for i in d["env_ids"]]
    assert ids == [0, 7] and E > 7
    src = np.zeros(E, dtype=np.int64)
    src[7] = 1
    return d["grid0"][src], d["pos0"][src], np.ascontiguousarray(d["actions"][:, src]), ids


# ---------------------------------------------------------------------------------------------------------------- plain movers
# name, spec, envs, options, (family, lanes, specialised), kernel name prefix: the rows of test_gpu_iowa.FAMILIES
FAMILIES = [
    ("step_fast specialised", lambda: I.iowa_spec(20, 20, 2, 2, 0.01, 21), 4096, {}, (N.FAMILY_WAVE, 64, 1), "step_fast<true, 2, 8, 2, 20, 20"),
    ("step_fast prebuilt", lambda: I.iowa_spec(20, 20, 2, 2, 0.01, 22), 4096, {"jit": 0}, (N.FAMILY_WAVE, 64, 0), "step_fast<true, 0, 0, 0, 0, 0"),
    ("step_big", lambda: I.iowa_spec(72, 72, 2, 2, 0.01, 23, direct=True), 256, {}, (N.FAMILY_WORKGROUP, 256, 1), "step_big<"),
    ("step_big prebuilt", lambda: I.iowa_spec(72, 72, 2, 2, 0.01, 24, direct=True), 256, {"jit": 0}, (N.FAMILY_WORKGROUP, 256, 0), "step_big<"),
    ("generic, a workgroup per env", lambda: I.iowa_spec(72, 72, 2, 2, 0.01, 25), 256, {"force_generic": 1}, (N.FAMILY_GENERIC, 256, 1), "step_kernel<256"),
    ("generic, a wave per env", lambda: I.iowa_spec(9, 9, 2, 2, 0.10, 26), 64, {"force_generic": 1}, (N.FAMILY_GENERIC, 64, 1), "step_kernel<64"),
    ("generic, packed", lambda: I.iowa_spec(20, 20, 2, 2, 0.01, 27, direct=True), 4096, {}, (N.FAMILY_GENERIC, 32, 1), "step_kernel<32"),
]
FAMILY_TURNS = (12, 12)      # device-drawn turns, then given ones


def family_world(case):
    ws = case[1]()
    if ws.height >= 72:
        ws.spawn_prob[1] = 0.02            # (two agents on 4 900 cells: enough decks to meet within the turns played)
    return ws


def given_actions(ws, E, T, seed, bad=0.01):
    """[T, E, A] uint8: uniform moves, a few indices outside the ActionSpec (nothing found, nothing counted)."""
    rng = np.random.default_rng(seed)
    act = rng.integers(0, ws.num_actions, size=(T, E, ws.num_agents)).astype(np.uint8)
    act[rng.random(act.shape) < bad] = 9
    return act


_FAMILY_RUNS = {}


def family_expected(case):
    """``(first, second, given)`` of a FAMILIES row: the checker's run of the device-drawn turns from a reset of epoch 0, and of the given turns
    that follow.  Computed once per process and shared."""
    name, E = case[0], case[2]
    if name not in _FAMILY_RUNS:
        ws = family_world(case)
        T1, T2 = FAMILY_TURNS
        given = given_actions(ws, E, T2, seed=E + T2)
        first = expected_counts(ws, IOWA_SLOTS, len(IOWA_KINDS), E, T1)
        second = expected_counts(ws, IOWA_SLOTS, len(IOWA_KINDS), E, T2, actions=given, first_turn=T1 + 1, start=(first["grid"], first["pos"]))
        _FAMILY_RUNS[name] = (first, second, given)
    return _FAMILY_RUNS[name]


# the worlds of test_gpu_iowa.ENTRY_WORLDS (one launch per rollout where the plan has the turn loop)
ENTRY_WORLDS = [("fast", lambda: I.iowa_spec(12, 10, 3, 2, 0.08, 31), 96), ("generic", lambda: I.iowa_spec(9, 9, 2, 2, 0.10, 32), 64),
                ("big", lambda: I.iowa_spec(72, 72, 3, 2, 0.03, 33, direct=True), 48)]


def many_agents_world():
    """``many_agents_80_treasurehunt``'s world (24 x 26, 80 agents): the instance that serves 65 .. 128 agents."""
    _d, spec = H.load_golden("many_agents_80_treasurehunt")
    return H.world_spec(spec)


def kind_slots(kinds_of_types, record):
    """What ``Environment.record_encounters`` means, restated: True = one slot per distinct kind in order of first appearance; a sequence of
    names = those slots in that order, every other kind uncounted."""
    kinds = tuple(dict.fromkeys(kinds_of_types)) if record is True else tuple(record)
    return kinds, [kinds.index(k) if k in kinds else NO_SLOT for k in kinds_of_types]
