"""CPU checks of encounter counts: the ABI, the checker (tests/encounters_common.py) against the fixture the reference's own
``CleanupAgent.act`` produced, what the worlds the GPU tests play contain, and how kinds fold onto slots."""
import os

import numpy as np
import pytest

from tests import encounters_common as X
from tests import helpers as H
from tests import iowa_common as I
from sorrel_amd import _native as N


def test_symbol_is_declared_and_exported():
    header = open(os.path.join(H.ROOT, "include", "sgw.h")).read()
    assert "int sgw_bind_encounters(sgw_engine* eng, int64_t* counts, const uint8_t* slot_of_type, int32_t num_slots);" in header
    assert "#define SGW_NO_SLOT 255" in header and N.NO_SLOT == 255
    assert "sgw_bind_encounters" in N.EXPORTS
    lib = N.load()
    assert hasattr(lib, "sgw_bind_encounters")
    assert lib.sgw_version() == b"sgw 0.3 (gfx950)"
    assert lib.sgw_bind_encounters(None, None, None, 0) == N.EINVAL          # a NULL engine is refused, not dereferenced


@pytest.fixture(scope="module")
def fixture_run():
    d, ws = X.load_fixture()
    g0, p0, acts, ids = X.fixture_batch(d)
    T = acts.shape[0]
    return d, ws, X.expected_counts(ws, X.CLEANUP_SLOTS, len(X.CLEANUP_KINDS), 8, T, actions=acts, start=(g0, p0))


def test_checker_equals_the_reference_turn_by_turn(fixture_run):
    d, ws, exp = fixture_run
    assert tuple(str(k) for k in d["kinds"]) == X.CLEANUP_KINDS and ws.agent_rule == N.AGENT_RULE_CLEANUP and ws.layers == 3
    ref = d["encounters"]                                                  # [T, 2, A, K], cumulative
    assert ref.shape == (40, 2, ws.num_agents, 9) and ref.dtype == np.int64
    for t in range(ref.shape[0]):
        assert np.array_equal(exp["cum"][t][[0, 7]], ref[t]), f"turn {t + 1}"
    # the step-loop fixture of the same run ends on the same grid
    old = np.load(os.path.join(H.GOLDEN_DIR, "cleanup_15x16.npz"))
    assert np.array_equal(exp["grid"][[0, 7]], old["grid"][-1]) and np.array_equal(exp["actions"][:, [0, 7]], old["actions"])


def test_the_fixture_world_can_catch_a_lost_increment(fixture_run):
    d, ws, exp = fixture_run
    ref_inc = np.diff(np.concatenate([np.zeros_like(d["encounters"][:1]), d["encounters"]]), axis=0)
    assert (ref_inc.sum(axis=-1) == ws.layers).all()                        # every act finds one entity per layer
    totals = dict(zip(X.CLEANUP_KINDS, d["encounters"][-1].sum(axis=(0, 1)).tolist()))
    assert totals == {"EmptyEntity": 630, "Wall": 48, "River": 17, "Pollution": 8, "AppleTree": 55, "Apple": 17, "CleanBeam": 38, "ZapBeam": 38,
                      "CleanupAgent": 109}
    assert all(n >= 1 for n in totals.values())
    assert int((ref_inc.max(axis=-1) >= 2).sum()) == 264 and int((ref_inc.max(axis=-1) == 3).sum()) == 94
    # ... and so can the batch of eight the GPU tests play
    assert (exp["inc"].max(axis=-1) == 3).any() and (exp["cum"][-1].sum(axis=(0, 1)) >= 1).all()


@pytest.mark.parametrize("case", X.FAMILIES, ids=[c[0] for c in X.FAMILIES])
def test_move_traces_contain_what_they_must(case):
    ws, E = X.family_world(case), case[2]
    first, second, given = X.family_expected(case)
    T1, T2 = X.FAMILY_TURNS
    assert (given >= ws.num_actions).any()                                   # an invalid action
    # the same turns through the Iowa checker: which type every agent found, what it was worth
    a = I.expected_run(ws, E, T1, want_obs=False)
    b = I.expected_run(ws, E, T2, actions=given, first_turn=T1 + 1, start=(a["grid"][-1], a["pos"][-1], a["total_reward"][-1]), want_obs=False)
    tt = np.concatenate([a["target_types"], b["target_types"]])
    assert np.array_equal(a["grid"][-1], first["grid"]) and np.array_equal(b["grid"][-1], second["grid"])
    found = tt != I.NO_TARGET
    slots = np.asarray(X.IOWA_SLOTS + [X.NO_SLOT] * (256 - len(X.IOWA_SLOTS)))[tt]
    assert (found & (slots == X.NO_SLOT)).any()                              # a target that is not counted
    assert (~found).any()
    cov = I.coverage(dict(target_types=tt, rewards=np.concatenate([a["rewards"], b["rewards"]])))
    assert all(plain >= 1 and loss >= 1 for plain, loss in cov["pairs"].values()), cov
    # two independent routes to the same counts: the slot of the type found, and the checker's value swap
    inc = np.concatenate([first["inc"], second["inc"]])
    mine = np.stack([(found & (slots == s)) for s in range(len(X.IOWA_KINDS))], axis=-1).astype(np.int64)
    assert np.array_equal(inc, mine)
    assert (inc.sum(axis=(0, 1, 2)) >= 1).all(), inc.sum(axis=(0, 1, 2))      # every slot, Wall included


def test_kinds_fold_onto_slots():
    from sorrel_amd.examples.cleanup.env import CleanupEnv
    from sorrel_amd.examples.iowa.entities import DECK_KINDS
    from sorrel_amd.examples.iowa.env import GamblingEnv

    assert GamblingEnv.record_encounters == tuple(DECK_KINDS) and GamblingEnv.record_targets and CleanupEnv.record_encounters is True
    assert not hasattr(GamblingEnv, "_fold_table") and "rollout" not in GamblingEnv.__dict__ and "_end_of_turn" not in GamblingEnv.__dict__
    # a registry as the Iowa example's: Sand, the spawner, Wall, fresh and drawn twins of every deck, the agent
    kinds = ["Sand", "EmptyEntity", "Wall"] + list(DECK_KINDS) * 2 + ["GamblingAgent"]
    assert X.kind_slots(kinds, tuple(DECK_KINDS)) == (tuple(DECK_KINDS), [255, 255, 255, 0, 1, 2, 3, 0, 1, 2, 3, 255])
    assert X.kind_slots(kinds, True) == (("Sand", "EmptyEntity", "Wall") + tuple(DECK_KINDS) + ("GamblingAgent",), [0, 1, 2, 3, 4, 5, 6, 3, 4, 5, 6, 7])

    class Proto:
        def __init__(self, kind):
            self.kind = kind

    class Registry:
        prototypes = [Proto(k) for k in kinds]

    class World:
        registry = Registry()

    from sorrel_amd.environment import Environment

    class Env(Environment):
        def setup_agents(self):
            pass

        def populate_environment(self):
            pass

    for record in (True, tuple(DECK_KINDS), ["Wall", "DeckC"]):
        env = Env.__new__(Env)
        env.world, env.record_encounters = World(), record
        assert env._encounter_slots() == X.kind_slots(kinds, record), record
    env.record_encounters = ["Wall", "Wall"]
    with pytest.raises(ValueError):
        env._encounter_slots()
    # the Cleanup worlds of the fixtures: Sand folds onto EmptyEntity, the two ages of a beam onto one slot
    ck = ["EmptyEntity", "EmptyEntity", "Wall", "River", "Pollution", "AppleTree", "Apple", "CleanBeam", "CleanBeam", "ZapBeam", "ZapBeam", "CleanupAgent"]
    assert X.kind_slots(ck, True) == (X.CLEANUP_KINDS, X.CLEANUP_SLOTS)
