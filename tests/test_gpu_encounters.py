"""GPU checks of encounter counts (``sgw_bind_encounters``): every acting path against tests/encounters_common.py (the unedited oracle with
0 / 1 values, once per slot) and against the counts the reference's own ``CleanupAgent.act`` kept.  Exact integer equality everywhere; all
worlds are small; counts are compared after every turn unless a test says otherwise."""
import numpy as np
import pytest

from tests import encounters_common as X
from tests import helpers as H
from tests import iowa_common as I
from tests.gpu_common import make_engine, torch_cuda  # noqa: F401
from sorrel_amd import _native as N

pytestmark = pytest.mark.gpu


def _np(t):
    return t.cpu().numpy()


def _start(torch, eng, grid, pos):
    eng.grid.copy_(torch.from_numpy(np.ascontiguousarray(grid)))
    eng.agent_pos.copy_(torch.from_numpy(np.ascontiguousarray(pos)))
    eng.total_reward.zero_()


# ---------------------------------------------------------------------------------------------------------------- 1 plain movers
@pytest.mark.parametrize("case", X.FAMILIES, ids=[c[0] for c in X.FAMILIES])
def test_move_every_family(torch_cuda, case):
    """A batch that reaches each kernel family (the plan says which, and is asserted): 12 device-drawn turns, then 12 given ones with bad
    actions among them; the four deck kinds and Wall are counted, everything else is not."""
    torch = torch_cuda
    name, _make, E, opts, (family, lanes, specialised), prefix = case
    ws = X.family_world(case)
    with N.options(**opts):
        plan = N.plan(ws.to_config(E, 0))
        assert (plan["family"], plan["lanes_per_env"], plan["specialised"]) == (family, lanes, specialised), plan
        assert plan["kernel"].startswith(prefix), plan["kernel"]
        eng = make_engine(ws, E)
        enc = eng.bind_encounters(X.IOWA_SLOTS, len(X.IOWA_KINDS))
        eng.reset(epoch=0)
    assert enc is eng.encounters and tuple(enc.shape) == (E, ws.num_agents, 5) and enc.dtype == torch.int64 and int(enc.sum()) == 0
    assert f"specialised={specialised}" in eng.launch_info()
    first, second, given = X.family_expected(case)
    T1, T2 = X.FAMILY_TURNS
    for k in range(T1):
        eng.step(random_actions=True, turn=k + 1)
        assert np.array_equal(_np(eng.actions), first["actions"][k]), f"{name}: actions differ at turn {k + 1}"
        assert np.array_equal(_np(enc), first["cum"][k]), f"{name}: counts differ at turn {k + 1}"
    for k in range(T2):
        eng.step(torch.from_numpy(given[k]).cuda(), turn=T1 + 1 + k)
        assert np.array_equal(_np(enc), first["cum"][-1] + second["cum"][k]), f"{name}: counts differ at given turn {k + 1}"
    assert np.array_equal(_np(eng.grid), second["grid"]) and np.array_equal(_np(eng.agent_pos), second["pos"])


def test_move_80_agents(torch_cuda):
    """The instance that serves 65 .. 128 agents (a ticket per agent group): its own copy of the act."""
    ws = X.many_agents_world()
    E, T = 8, 6
    assert ws.num_agents == 80 and ws.num_types == len(X.TH_SLOTS)
    eng = make_engine(ws, E)
    assert "step_kernel<256" in eng.launch_info(), eng.launch_info()
    enc = eng.bind_encounters(X.TH_SLOTS, len(X.TH_KINDS))
    eng.reset(epoch=0)
    exp = X.expected_counts(ws, X.TH_SLOTS, len(X.TH_KINDS), E, T)
    assert (exp["cum"][-1].sum(axis=(0, 1)) >= 1).all()
    for k in range(T):
        eng.step(random_actions=True, turn=k + 1)
        assert np.array_equal(_np(enc), exp["cum"][k]), f"turn {k + 1}"
    assert np.array_equal(_np(eng.grid), exp["grid"])


# ---------------------------------------------------------------------------------------------------------------- 2 one launch
@pytest.mark.parametrize("case", X.ENTRY_WORLDS, ids=[c[0] for c in X.ENTRY_WORLDS])
def test_rollout_counts_every_turn(torch_cuda, case):
    """``eng.rollout(T)``: the turn loop inside one launch where the plan has it (with observations), a loop of launches otherwise -- the counts
    are the checker's 16-turn sum either way, and a second rollout goes on from there."""
    torch = torch_cuda
    _name, make, E = case
    ws = make()
    T, K = 16, len(X.IOWA_KINDS)
    given = X.given_actions(ws, E, 2 * T, seed=5)
    one = X.expected_counts(ws, X.IOWA_SLOTS, K, E, T, actions=given[:T])
    two = X.expected_counts(ws, X.IOWA_SLOTS, K, E, T, actions=given[T:], first_turn=T + 1, start=(one["grid"], one["pos"]))
    assert one["cum"][-1].sum() > 0 and two["cum"][-1].sum() > 0
    for write_obs in (True, False):
        eng = make_engine(ws, E)
        enc = eng.bind_encounters(X.IOWA_SLOTS, K)
        eng.reset(epoch=0)
        eng.rollout(T, actions=torch.from_numpy(given[:T]).cuda(), write_obs=write_obs)
        assert np.array_equal(_np(enc), one["cum"][-1]), f"write_obs={write_obs}"
        eng.rollout(T, actions=torch.from_numpy(given[T:]).cuda(), write_obs=write_obs)
        assert np.array_equal(_np(enc), one["cum"][-1] + two["cum"][-1]), f"write_obs={write_obs}, second rollout"
        assert np.array_equal(_np(eng.grid), two["grid"])
    # the engine's own draws
    free = X.expected_counts(ws, X.IOWA_SLOTS, K, E, T)
    eng = make_engine(ws, E)
    enc = eng.bind_encounters(X.IOWA_SLOTS, K)
    eng.reset(epoch=0)
    eng.rollout(T, random_actions=True)
    assert np.array_equal(_np(enc), free["cum"][-1]) and np.array_equal(_np(eng.grid), free["grid"])


def test_rollout_across_an_epoch_boundary(torch_cuda):
    """``set_auto_reset``: the reset at the end of turn 10 starts epoch 1; the counts run on across it."""
    _name, make, E = X.ENTRY_WORLDS[0]
    ws = make()
    T, K = 16, len(X.IOWA_KINDS)
    exp = X.expected_counts(ws, X.IOWA_SLOTS, K, E, T, auto_reset=10)
    assert exp["inc"][:10].sum() > 0 and exp["inc"][10:].sum() > 0
    eng = make_engine(ws, E)
    enc = eng.bind_encounters(X.IOWA_SLOTS, K)
    eng.set_auto_reset(10)
    eng.reset(epoch=0)
    eng.rollout(T, random_actions=True)
    assert (eng.epoch, eng.turn) == (1, 6)
    assert np.array_equal(_np(enc), exp["cum"][-1]) and np.array_equal(_np(eng.grid), exp["grid"])
    eng.reset(epoch=5)                                     # sgw_reset leaves them alone as well
    assert np.array_equal(_np(enc), exp["cum"][-1])


# ---------------------------------------------------------------------------------------------------------------- 3 Cleanup
E_FIX = 70      # the fixture's two envs in a batch of 70: more than one workgroup on every plan, the last one partly filled


@pytest.fixture(scope="module")
def cleanup_run():
    d, ws = X.load_fixture()
    g0, p0, acts, _ids = X.fixture_batch(d, E_FIX)
    exp = X.expected_counts(ws, X.CLEANUP_SLOTS, len(X.CLEANUP_KINDS), E_FIX, acts.shape[0], actions=acts, start=(g0, p0))
    assert (exp["inc"].max(axis=-1) == 3).any() and (exp["cum"][-1].sum(axis=(0, 1)) >= 1).all()
    return d, ws, g0, p0, acts, exp


CLEANUP_PLANS = [("default", {}, N.FAMILY_WAVE, 1), ("force_generic", {"force_generic": 1}, N.FAMILY_GENERIC, 1), ("jit=0", {"jit": 0}, N.FAMILY_WAVE, 0)]


@pytest.mark.parametrize("case", CLEANUP_PLANS, ids=[c[0] for c in CLEANUP_PLANS])
def test_cleanup_fixture_replay(torch_cuda, cleanup_run, case):
    """The reference's run from its ``grid0`` / ``pos0`` with its actions: every env against the checker, envs 0 and 7 against the counts the
    reference's agents kept -- on the default plan (a wave per env with the rule tables), the generic kernel and the prebuilt instances."""
    torch = torch_cuda
    d, ws, g0, p0, acts, exp = cleanup_run
    _name, opts, family, specialised = case
    with N.options(**opts):
        plan = N.plan(ws.to_config(E_FIX, 0))
        assert (plan["family"], plan["specialised"]) == (family, specialised), plan
        if family == N.FAMILY_WAVE:
            assert plan["rules"] == 1 and plan["kernel"].startswith("step_fast<"), plan
        eng = make_engine(ws, E_FIX)
        enc = eng.bind_encounters(X.CLEANUP_SLOTS, len(X.CLEANUP_KINDS))
    _start(torch, eng, g0, p0)
    ref = d["encounters"]
    for k in range(acts.shape[0]):
        eng.step(torch.from_numpy(acts[k]).cuda(), turn=k + 1)
        mine = _np(enc)
        assert np.array_equal(mine, exp["cum"][k]), f"turn {k + 1}"
        assert np.array_equal(mine[[0, 7]], ref[k]), f"turn {k + 1}: not the reference's counts"
    assert np.array_equal(_np(eng.grid), exp["grid"]) and np.array_equal(_np(eng.agent_dir), exp["agent_dir"])
    # ... and the same 40 turns as one rollout
    eng2 = make_engine(ws, E_FIX)
    enc2 = eng2.bind_encounters(X.CLEANUP_SLOTS, len(X.CLEANUP_KINDS))
    _start(torch, eng2, g0, p0)
    eng2.rollout(acts.shape[0], actions=torch.from_numpy(acts).cuda())
    assert np.array_equal(_np(enc2), exp["cum"][-1])


def test_cleanup_workgroup_per_env(torch_cuda):
    """72 Cleanup agents on 30 x 34: the planner's generic kernel with a workgroup per env, whose agent groups run their own copy of the act."""
    ws = H.world_spec(H.load_golden("cleanup_15x16")[1])
    A, E, T = 72, 10, 5
    ws.height, ws.width, ws.num_agents, ws.agent_type = 30, 34, A, [ws.agent_type[0]] * A
    eng = make_engine(ws, E, first=2)
    assert "step_kernel<256" in eng.launch_info(), eng.launch_info()
    enc = eng.bind_encounters(X.CLEANUP_SLOTS, len(X.CLEANUP_KINDS))
    eng.reset(epoch=1)
    exp = X.expected_counts(ws, X.CLEANUP_SLOTS, len(X.CLEANUP_KINDS), E, T, epoch=1, first_env_id=2, agent_dir=_np(eng.agent_dir))
    assert (exp["inc"].sum(axis=-1) <= 3).all() and (exp["inc"].max(axis=-1) >= 2).any()
    for k in range(T):
        eng.step(random_actions=True, turn=k + 1)
        assert np.array_equal(_np(enc), exp["cum"][k]), f"turn {k + 1}"
    assert np.array_equal(_np(eng.grid), exp["grid"])


@pytest.mark.parametrize("with_rows", [True, False], ids=["window rows", "no rows"])
def test_cleanup_through_sgw_act(torch_cuda, cleanup_run, with_rows):
    """The sweep and every window once, then ``sgw_act`` agent after agent -- with the later agents' windows to keep current, and without."""
    torch = torch_cuda
    _d, ws, g0, p0, acts, exp = cleanup_run
    eng = make_engine(ws, E_FIX)
    enc = eng.bind_encounters(X.CLEANUP_SLOTS, len(X.CLEANUP_KINDS))
    _start(torch, eng, g0, p0)
    rows = eng.window_rows(None) if with_rows else None
    for k in range(12):
        ta = torch.from_numpy(acts[k]).cuda()
        eng.step(ta, sweep=True, no_move=True, turn=k + 1)
        for a in range(ws.num_agents):
            eng.act(a, rows, action=ta[:, a].to(torch.int64).contiguous())
        assert np.array_equal(_np(enc), exp["cum"][k]), f"turn {k + 1}"


def test_move_through_sgw_act_and_phases(torch_cuda):
    """Plain movers agent after agent: ``sgw_act``, and a phase of ``sgw_step`` per agent."""
    torch = torch_cuda
    _name, make, E = X.ENTRY_WORLDS[0]
    ws = make()
    T, K, A = 10, len(X.IOWA_KINDS), ws.num_agents
    given = X.given_actions(ws, E, T, seed=6)
    exp = X.expected_counts(ws, X.IOWA_SLOTS, K, E, T, actions=given)
    eng, eng2 = make_engine(ws, E), make_engine(ws, E)
    enc, enc2 = eng.bind_encounters(X.IOWA_SLOTS, K), eng2.bind_encounters(X.IOWA_SLOTS, K)
    eng.reset(epoch=0)
    eng2.reset(epoch=0)
    rows = eng.window_rows(None)
    for k in range(T):
        ta = torch.from_numpy(given[k]).cuda()
        eng.turn_set(0, k)
        eng.step(ta, sweep=True, no_move=True, turn=k + 1)
        eng2.step(sweep=True, agent_begin=0, agent_end=0, write_obs=False, turn=k + 1)
        for a in range(A):
            eng.act(a, rows, action=ta[:, a].to(torch.int64).contiguous())
            eng2.step(ta, sweep=False, write_obs=False, agent_begin=a, agent_end=a + 1, turn=k + 1)
        assert np.array_equal(_np(enc), exp["cum"][k]), f"sgw_act, turn {k + 1}"
        assert np.array_equal(_np(enc2), exp["cum"][k]), f"per-agent sgw_step, turn {k + 1}"


# ---------------------------------------------------------------------------------------------------------------- 4 guards
def test_sentinels_unbinding_and_refusals(torch_cuda):
    torch = torch_cuda
    _name, make, E = X.ENTRY_WORLDS[0]
    ws = make()
    K, A = len(X.IOWA_KINDS), ws.num_agents
    eng = make_engine(ws, E)
    before = eng.launch_info()
    caps = eng.capabilities()
    # the counts inside a larger buffer: the elements on both sides stay as they are
    pad = 64
    buf = torch.full((pad + E * A * K + pad,), -7, dtype=torch.int64, device="cuda:0")
    counts = buf[pad:pad + E * A * K].view(E, A, K)
    counts.zero_()
    assert eng.bind_encounters(X.IOWA_SLOTS, K, counts=counts) is counts
    eng.reset(epoch=0)
    T = 8
    exp = X.expected_counts(ws, X.IOWA_SLOTS, K, E, T)
    eng.rollout(T, random_actions=True)
    assert np.array_equal(_np(counts), exp["cum"][-1]) and exp["cum"][-1].sum() > 0
    assert bool((buf[:pad] == -7).all()) and bool((buf[pad + E * A * K:] == -7).all())
    # unbound: nothing is written, and the engine launches what it launched before
    eng.bind_encounters(None)
    assert eng.encounters is None and eng.launch_info() == before and eng.capabilities() == caps
    eng.rollout(4, random_actions=True)
    eng.step(random_actions=True)
    assert np.array_equal(_np(counts), exp["cum"][-1])
    # what the library refuses
    with pytest.raises(ValueError):
        eng.bind_encounters([K] + X.IOWA_SLOTS[1:], K)                    # a slot that is neither below num_slots nor NO_SLOT
    with pytest.raises(ValueError):
        eng.bind_encounters(X.IOWA_SLOTS, 33, counts=torch.zeros((E, A, 33), dtype=torch.int64, device="cuda:0"))
    with pytest.raises(ValueError):
        eng.bind_encounters(X.IOWA_SLOTS, 0)
    with pytest.raises(ValueError):
        eng.bind_encounters(X.IOWA_SLOTS[:-1], K)
    lib = N.load()
    table = bytes(X.IOWA_SLOTS)
    assert lib.sgw_bind_encounters(eng._h, counts.data_ptr() + 4, table, K) == N.EINVAL        # misaligned
    assert lib.sgw_bind_encounters(eng._h, counts.data_ptr(), table, 33) == N.EINVAL
    assert lib.sgw_bind_encounters(eng._h, counts.data_ptr(), bytes([K] + X.IOWA_SLOTS[1:]), K) == N.EINVAL
    assert eng.launch_info() == before                                     # ... before anything changes
    eng.step(random_actions=True)
    assert np.array_equal(_np(counts), exp["cum"][-1])
    tag = H.world_spec(H.load_golden("tag_9x9")[1])
    teng = make_engine(tag, 16)
    with pytest.raises(ValueError):
        teng.bind_encounters([0] * tag.num_types, 1)
    # no speculative resolve while counts are bound (a pass replays acts)
    from sorrel_amd.spec import treasurehunt_spec
    th = treasurehunt_spec(16, 16, 4, 2, spawn_prob=0.1, seed=3)
    e2 = make_engine(th, 32)
    assert e2.capabilities() & N.CAP_RESOLVE
    e2.bind_encounters(X.TH_SLOTS, len(X.TH_KINDS))
    assert not (e2.capabilities() & N.CAP_RESOLVE)
    e2.bind_encounters(None)
    assert e2.capabilities() & N.CAP_RESOLVE


# ---------------------------------------------------------------------------------------------------------------- 5 the examples
def _linear_policy(torch, E, memory=6):
    from sorrel_amd.models import BaseModel

    class Policy(BaseModel):
        """A fixed linear layer + argmax: deterministic, capturable (no host synchronisation)."""

        def __init__(self, input_size, action_space):
            super().__init__(input_size, action_space, memory_size=memory, num_envs=E, device="cuda:0")
            n = int(np.prod(input_size))
            g = torch.Generator().manual_seed(977 + n)
            self.weight = torch.randn((n, action_space), generator=g).cuda()

        def take_action(self, state):
            return (state.reshape(state.shape[0], -1) @ self.weight).argmax(dim=1)

    return Policy


def _cleanup_env(torch, E, policy=True, seed=3):
    from sorrel_amd.examples.cleanup.entities import EmptyEntity
    from sorrel_amd.examples.cleanup.env import CleanupEnv
    from sorrel_amd.examples.cleanup.main import make_config
    from sorrel_amd.examples.cleanup.world import CleanupWorld

    cfg = make_config(height=15, width=16, num_agents=4, vision=3, beam_radius=3, max_turns=30)
    cfg["env"].update(initial_apples=6, apple_spawn_chance=0.03, pollution_spawn_chance=0.06)
    return CleanupEnv(CleanupWorld(config=cfg, default_entity=EmptyEntity(), num_envs=E, device="cuda:0", seed=seed), cfg,
                      model_factory=_linear_policy(torch, E) if policy else None)


def _expected_for_env(env, acts, start, first_turn):
    ws = env.compile_spec()
    kinds, slots = X.kind_slots([p.kind for p in env.world.registry.prototypes], env.record_encounters)
    assert kinds == tuple(env.encounter_kinds)
    return X.expected_counts(ws, slots, len(kinds), env.num_envs, len(acts), epoch=env.epoch, actions=np.stack(acts), first_turn=first_turn,
                             start=start[:2], agent_dir=start[2])


def test_cleanup_example(torch_cuda):
    torch = torch_cuda
    E, T = 32, 12
    eager, rec, spec = _cleanup_env(torch, E), _cleanup_env(torch, E), _cleanup_env(torch, E)
    kinds = eager.encounter_kinds
    assert eager.record_encounters is True and sorted(kinds) == sorted(X.CLEANUP_KINDS)      # (Sand folds onto EmptyEntity, the beams' ages onto one slot)
    eng = eager._ensure_engine()
    assert eager.encounters is eng.encounters and tuple(eager.encounters.shape) == (E, 4, 9) and int(eager.encounters.sum()) == 0
    start = (_np(eng.grid), _np(eng.agent_pos), _np(eng.agent_dir))
    acts = []
    for _ in range(T):
        eager.take_turn()
        acts.append(_np(eager.actions))
    exp = _expected_for_env(eager, acts, start, 1)
    assert np.array_equal(_np(eager.encounters), exp["cum"][-1]) and (exp["inc"].max(axis=-1) >= 2).any()
    for a, agent in enumerate(eager.agents):
        assert np.array_equal(_np(agent.encounters), exp["cum"][-1][:, a])
        for e in (0, E - 1):
            want = {k: int(n) for k, n in zip(kinds, exp["cum"][-1][e, a]) if n}
            assert agent.encounter_dict(e) == want and sum(want.values()) == 3 * T
    # a recorded turn carries the increments inside the graph
    cap = rec.capture_turn(warmup=2, force=True)
    assert cap is not None, getattr(rec, "capture_error", None)
    for _ in range(T - 2):
        rec.take_turn()
    assert rec.turn == T and cap.turns_replayed == T - 2
    assert np.array_equal(_np(rec.encounters), exp["cum"][-1]) and np.array_equal(_np(rec.world.grid), _np(eager.world.grid))
    # speculate_turns = "always": no sgw_turn_resolve while counts are bound (its passes replay acts).  The generic speculative turn plays whole
    # turns on a scratch handle and carries the counts as state, so whichever loop plays, an act is counted once
    spec.speculate_turns = "always"
    assert not (spec._ensure_engine().capabilities() & N.CAP_RESOLVE)
    for _ in range(T):
        spec.take_turn()
        assert spec.turn_plan()["loop"] != "speculative" or spec._spec_generic is True
    assert np.array_equal(_np(spec.encounters), exp["cum"][-1]) and np.array_equal(_np(spec.world.grid), _np(eager.world.grid))
    # never cleared by reset(), as in the reference; clear_encounters() is the caller's decision
    eager.reset()
    assert np.array_equal(_np(eager.encounters), exp["cum"][-1])
    eager.clear_encounters()
    assert int(eager.encounters.sum()) == 0 and eager.agents[0].encounter_dict() == {}


def _iowa_env(E, seed=2, max_turns=40):
    from sorrel_amd.examples.iowa.entities import EmptyEntity
    from sorrel_amd.examples.iowa.env import GamblingEnv
    from sorrel_amd.examples.iowa.main import make_config
    from sorrel_amd.examples.iowa.world import GamblingWorld

    cfg = make_config(spawn_prob=0.05, epochs=0, max_turns=max_turns)
    return GamblingEnv(GamblingWorld(cfg, EmptyEntity(), num_envs=E, device="cuda:0", seed=seed), cfg)


def test_iowa_example_rolls_out_in_one_call(torch_cuda):
    """Device-random agents: ``env.rollout(20)`` is ``Environment.rollout`` -- the launches ``GridEngine.rollout(20)`` issues on the same
    world, not 20 turns of Python -- and counts what 20 ``take_turn()``s count."""
    E, T = 64, 20
    loop, fused = _iowa_env(E), _iowa_env(E)
    assert tuple(fused.encounters.shape) == (E, 2, 4) and fused.encounter_kinds == I.DECK_KINDS
    for _ in range(T):
        loop.take_turn()
    feng = fused._ensure_engine()
    feng.set_timing(True)
    fused.rollout(T)
    _ms, launches = feng.step_time_ms()
    assert fused.turn == T and np.array_equal(_np(fused.encounters), _np(loop.encounters)) and int(fused.encounters.sum()) > 0
    assert np.array_equal(_np(fused.world.grid), _np(loop.world.grid)) and np.array_equal(_np(fused.world.total_reward), _np(loop.world.total_reward))
    assert fused.encounters is feng.encounters and np.array_equal(_np(fused.agents[1].encounters), _np(fused.encounters)[:, 1])
    # the same world on a bare engine: as many launches
    bare = make_engine(fused.compile_spec(), E)
    bare.reset(epoch=fused.epoch)
    bare.set_timing(True)
    bare.rollout(T, random_actions=True)
    _ms, bare_launches = bare.step_time_ms()
    assert launches == bare_launches, (launches, bare_launches)
    if N.plan(fused.compile_spec().to_config(E, 0))["rollout_in_one_launch"]:
        assert launches < T, launches
    # against the checker, in the example's own type numbering
    kinds, slots = X.kind_slots([p.kind for p in fused.world.registry.prototypes], fused.record_encounters)
    assert kinds == I.DECK_KINDS
    exp = X.expected_counts(fused.compile_spec(), slots, 4, E, T, epoch=fused.epoch)
    assert np.array_equal(_np(fused.encounters), exp["cum"][-1])
    fused.reset()                                                   # GamblingAgent.reset clears its counts, as the reference's does
    assert int(fused.encounters.sum()) == 0


def test_checkpoint_round_trip(torch_cuda):
    E = 16
    a, b = _iowa_env(E), _iowa_env(E)
    a.rollout(15)
    sd = a.state_dict()
    assert "encounters" in sd and sd["encounter_kinds"] == list(I.DECK_KINDS) and int(sd["encounters"].sum()) > 0
    b.load_state_dict(sd)
    assert np.array_equal(_np(b.encounters), _np(a.encounters))
    a.rollout(10)
    b.rollout(10)
    assert np.array_equal(_np(b.encounters), _np(a.encounters)) and np.array_equal(_np(b.world.grid), _np(a.world.grid))
    # an environment that records nothing carries nothing
    from tests.gpu_common import make_env
    th = make_env(12, 12, 2, 2, 8)
    assert th.encounters is None and "encounters" not in th.state_dict()
    with pytest.raises(ValueError):
        b.load_state_dict({k: v for k, v in sd.items() if k != "encounters"})
