"""CPU checks of drawn values and the Iowa Gambling Task example: the reference-generated fixtures against the independent
checker (tests/iowa_common.py), the example's compiled tables, the ABI suffix and what ``sgw_create`` rejects."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from tests import iowa_common as I
from sorrel_amd import _native as N
from sorrel_amd.entities import Entity
from sorrel_amd.entities.rules import DrawnValue
from sorrel_amd.examples.iowa import entities as ie
from sorrel_amd.examples.iowa.env import ENTITY_LIST, GamblingEnv
from sorrel_amd.examples.iowa.main import make_config
from sorrel_amd.examples.iowa.world import GamblingWorld
from sorrel_amd.spec import RULE_BECOME_IF, RULE_NONE, RULE_SPAWN, treasurehunt_spec

FIXTURES = ["iowa_12x10_three_agents", "iowa_20x20_default", "iowa_9x9_dense"]


class CpuGamblingEnv(GamblingEnv):
    """No GPU here: skip the device reset, keep everything else."""

    def spawn_agents(self):
        self.world.agent_layer = 1


def make_env(h=20, w=20, a=2, r=2, E=4, sp=0.01):
    cfg = make_config(h, w, a, r, spawn_prob=sp)
    return CpuGamblingEnv(GamblingWorld(cfg, ie.EmptyEntity(), num_envs=E, device="cpu", seed=5), cfg)


def test_fixtures_are_all_there():
    assert I.fixture_names() == FIXTURES


@pytest.mark.parametrize("name", FIXTURES)
def test_checker_reproduces_the_reference(name):
    """Every array the reference's own take_turn produced (plugin Deck / EmptyEntity on the counter RNG) equals what the checker forms from
    the unedited oracle (type ids as values) + the value tables + stream 8."""
    d, ws = I.load_fixture(name)
    E, T = int(d["num_envs"]), int(d["turns"])
    mine = I.expected_run(ws, E, T, actions=d["actions"])
    for key in ("grid0", "pos0", "grid", "pos", "obs", "actions", "rewards", "total_reward"):
        assert np.array_equal(d[key], mine[key]), key
    assert np.array_equal(d["target_kinds"], I.fold_kinds(mine["target_types"]))
    # the counter model's actions are the engine's own draws
    assert np.array_equal(I.expected_run(ws, E, T, want_obs=False)["actions"], d["actions"])
    # the hand-written tables are the ones the fixture was made with
    fresh = I.iowa_spec(ws.height, ws.width, ws.num_agents, ws.vision_radius, ws.spawn_prob[1], ws.seed)
    assert I.spec_to_json(fresh) == str(d["spec_json"])


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_exercise_the_rule(name):
    """Equality proves something only if every deck is stepped on with both outcomes and a deck is stepped on in the turn it was spawned
    (value 0, and still an encounter)."""
    d, ws = I.load_fixture(name)
    run = dict(target_types=I.expected_run(ws, int(d["num_envs"]), int(d["turns"]), actions=d["actions"], want_obs=False)["target_types"],
               rewards=d["rewards"])
    cov = I.coverage(run)
    assert cov["fresh"] >= 1
    for kind, (plain, loss) in cov["pairs"].items():
        assert plain >= 1 and loss >= 1, (kind, plain, loss)
    tt = run["target_types"]
    fresh = (tt >= I.FRESH0) & (tt < I.DRAWN0)
    assert np.all(d["rewards"][fresh] == 0.0) and np.all(d["target_kinds"][fresh] >= 0)     # reward 0, and it counts as an encounter
    assert int((d["target_kinds"] >= 0).sum()) == cov["fresh"] + cov["drawn"]


def test_deck_outcomes_in_the_reference_order():
    assert [ie.deck_outcomes(n) for n in ie.DECKS] == I.deck_tables()
    assert ie.deck_outcomes("a") == (1 + 0.1, (1 + -2.5) + 0.1, 0.5) and ie.deck_outcomes("d") == (0.5 + 0.1, (0.5 + -2.5) + 0.1, 0.1)


def test_compile_spec_of_the_example():
    env = make_env()
    s = env.compile_spec()
    assert s.num_types == 12 and s.num_channels == 8 and ENTITY_LIST == I.ENTITY_LIST
    ref = I.iowa_spec(20, 20, 2, 2, 0.01, seed=5)
    protos = env.world.registry.prototypes

    def tid(kind, drawn=None):
        hits = [t for t, p in enumerate(protos) if (p.kind == kind or type(p).__name__ == kind) and (drawn is None or getattr(p, "drawn", None) == drawn)]
        assert len(hits) == 1, (kind, drawn, hits)
        return hits[0]

    mine = [tid("Sand"), tid("EmptyEntity"), tid("Wall")] + [tid(k, False) for k in I.DECK_KINDS] + [tid(k, True) for k in I.DECK_KINDS] + [tid("GamblingAgent")]
    assert sorted(mine) == list(range(12))
    for rt, t in enumerate(mine):       # same semantics per type, whatever ids the registry handed out
        assert s.type_value[t] == ref.type_value[rt] and s.type_value_alt[t] == ref.type_value_alt[rt] and s.value_alt_prob[t] == ref.value_alt_prob[rt]
        assert s.type_passable[t] == ref.type_passable[rt] and s.type_rule[t] == ref.type_rule[rt]
        assert np.array_equal(s.appearance[t], ref.appearance[rt])
    for k in range(4):                  # fresh and drawn twins: one look, fresh -> drawn on the next sweep, unconditionally
        f, dr = mine[I.FRESH0 + k], mine[I.DRAWN0 + k]
        assert np.array_equal(s.appearance[f], s.appearance[dr]) and s.appearance[f].sum() == 1.0
        assert s.type_rule[f] == RULE_BECOME_IF and s.rule_become[f] == dr and s.rule_layer[f] == -1 and s.type_rule[dr] == RULE_NONE
        assert protos[dr].value == ie.deck_outcomes(ie.DECKS[k])[0]       # the host-side value is the outcome without the loss
    sp = mine[1]
    assert s.type_rule[sp] == RULE_SPAWN and s.spawn_prob[sp] == 0.01 and list(s.spawn_choices[sp]) == mine[I.FRESH0:I.DRAWN0]
    assert [s.layer_fill_type[0], s.layer_fill_type[1]] == [mine[0], mine[1]] and list(s.layer_border_type) == [mine[2], mine[2]]
    assert s.default_type == mine[1] and s.fill_type == mine[2] and s.agent_rule == 0 and s.has_drawn_values
    cfg = s.to_config(4, 0)
    assert cfg.num_types == 12 and [cfg.value_alt_prob[mine[I.DRAWN0 + k]] for k in range(4)] == [0.5, 0.1, 0.5, 0.1]
    assert env.record_targets and tuple(env.encounters.shape) == (4, 2, 4)
    # two specs, one plan family for the reference's shape: a wave per env with the rule tables
    plan = N.plan(s.to_config(4096, 0))
    assert plan["family"] == N.FAMILY_WAVE and plan["rules"] == 1


def test_zero_rule_specs_leave_the_suffix_zero():
    for ws in (treasurehunt_spec(32, 32, 8, 3), treasurehunt_spec(21, 21, 2, 2, seed=9)):
        cfg = ws.to_config(16, 0)
        assert not ws.has_drawn_values
        assert all(cfg.type_value_alt[t] == 0.0 and cfg.value_alt_prob[t] == 0.0 for t in range(N.MAX_TYPES))
    for name in H.golden_names():
        _d, ospec = H.load_golden(name)
        cfg = H.world_spec(ospec).to_config(4, 0)
        assert all(cfg.type_value_alt[t] == 0.0 and cfg.value_alt_prob[t] == 0.0 for t in range(N.MAX_TYPES)), name
    # a pure suffix: the struct grew by exactly the two tables, behind grid_env_stride
    assert N.SgwConfig.type_value_alt.offset == N.SgwConfig.grid_env_stride.offset + 8
    assert C.sizeof(N.SgwConfig) == N.SgwConfig.value_alt_prob.offset + 8 * N.MAX_TYPES
    assert N.load().sgw_version() == b"sgw 0.3 (gfx950)" and "sgw_bind_target_types" in N.EXPORTS


def test_create_time_rejections():
    """What sgw_create rejects, through sgw_plan (the same validation, host arithmetic)."""
    def cfg_of(**edit):
        ws = I.iowa_spec(12, 12, 2, 2, 0.05, 1)
        for k, v in edit.items():
            setattr(ws, k, v)
        return ws.to_config(8, 0)

    N.plan(cfg_of())
    c = cfg_of(); c.value_alt_prob[I.DRAWN0] = 1.5
    with pytest.raises(ValueError, match="value_alt_prob"):
        N.plan(c)
    c = cfg_of(); c.value_alt_prob[I.DRAWN0] = -0.1
    with pytest.raises(ValueError, match="value_alt_prob"):
        N.plan(c)
    c = cfg_of(); c.value_alt_prob[I.DRAWN0] = float("nan")
    with pytest.raises(ValueError, match="value_alt_prob"):
        N.plan(c)
    c = cfg_of(); c.type_value_alt[0] = float("inf")
    with pytest.raises(ValueError, match="type_value_alt"):
        N.plan(c)
    c = cfg_of(); c.value_alt_prob[I.AGENT_T] = 0.5
    with pytest.raises(ValueError, match="agent type"):
        N.plan(c)
    c = cfg_of(agent_rule=N.AGENT_RULE_TAG, tag_it_type=I.AGENT_T, tag_notit_type=2)
    with pytest.raises(ValueError, match="SGW_AGENT_RULE_MOVE"):
        N.plan(c)
    c = cfg_of(agent_rule=N.AGENT_RULE_CLEANUP, action_kind=[0, 0, 0, 0])
    with pytest.raises(ValueError, match="SGW_AGENT_RULE_MOVE"):
        N.plan(c)
    c = cfg_of(); c.value_alt_prob[I.DRAWN0] = 1.0; c.value_alt_prob[I.DRAWN0 + 1] = 0.0      # the ends of the range are fine
    N.plan(c)


def test_value_rules_fail_loudly_at_compile_time():
    class Lottery(Entity):
        def __init__(self, rule=None, value=0):
            super().__init__()
            self.passable = True
            self.kind = "DeckA"
            self.value = value
            if rule is not None:
                self.value_rule = rule

    for bad, msg in ((DrawnValue(1.0, lambda: 2.0, 0.5), "callable"), (DrawnValue(1.0, [2.0, 3.0], 0.5), "two outcomes"),
                     (DrawnValue(1.0, 2.0, 1.5), r"\[0, 1\]"), (DrawnValue(1.0, float("inf"), 0.5), "finite")):
        env = make_env(12, 12)
        env.world.add((3, 3, 1), Lottery(bad))
        with pytest.raises(ValueError, match=msg):
            env.compile_spec()
    env = make_env(12, 12)
    with pytest.raises(ValueError, match="callable"):         # a callable value: rejected as soon as the entity needs a type id
        env.world.add((3, 3, 1), Lottery(value=lambda: 1.0))
    # two entities with equal rules are one type; a different rule is another
    a, b, c = Lottery(DrawnValue(1.0, 2.0, 0.5)), Lottery(DrawnValue(1.0, 2.0, 0.5)), Lottery(DrawnValue(1.0, 2.0, 0.25))
    assert a.type_key() == b.type_key() != c.type_key() and Lottery().type_key() != a.type_key()
    assert ie.Deck("a").type_key() == ie.Deck("a").type_key() != ie.Deck("a", drawn=True).type_key()


def test_compat_maps_the_example():
    import sorrel_amd.compat as compat

    assert "examples.iowa" in compat.MIRRORED and "examples.iowa" not in compat.OUT_OF_SCOPE
