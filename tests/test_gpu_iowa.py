"""GPU checks of drawn values, ``target_types`` and the Iowa Gambling Task example.  Equality everywhere: the expected arrays come from
tests/iowa_common.py (the unedited oracle with type ids as values + the two value tables + stream 8 of the oracle's counter RNG)."""
import numpy as np
import pytest

from tests import iowa_common as I
from tests.gpu_common import make_engine, torch_cuda  # noqa: F401
from sorrel_amd import _native as N

pytestmark = pytest.mark.gpu

FIXTURES = ["iowa_12x10_three_agents", "iowa_20x20_default", "iowa_9x9_dense"]


def _np(t):
    return t.cpu().numpy()


def _bound(ws, E, **kw):
    eng = make_engine(ws, E, **kw)
    eng.bind_target_types(True)
    eng.reset(epoch=0)
    return eng


def _given_actions(ws, E, T, seed, bad=0.01):
    """[T, E, A] uint8: uniform moves, a few indices outside the ActionSpec (no target: 255, reward 0)."""
    rng = np.random.default_rng(seed)
    act = rng.integers(0, ws.num_actions, size=(T, E, ws.num_agents)).astype(np.uint8)
    act[rng.random(act.shape) < bad] = 9
    return act


def _assert_turn(eng, exp, k, what, obs=True):
    names = [("grid", eng.grid), ("pos", eng.agent_pos), ("actions", eng.actions), ("rewards", eng.rewards),
             ("total_reward", eng.total_reward), ("target_types", eng.target_types)]
    if obs:
        names.append(("obs", eng.obs))
    for name, mine in names:
        assert np.array_equal(_np(mine), exp[name][k]), f"{what}: {name} differs at turn {k + 1}"


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_through_sgw_step(torch_cuda, name):
    torch = torch_cuda
    d, ws = I.load_fixture(name)
    E, T = int(d["num_envs"]), int(d["turns"])
    exp = I.expected_run(ws, E, T, actions=d["actions"])
    eng = _bound(ws, E)
    assert np.array_equal(_np(eng.grid), d["grid0"]) and np.array_equal(_np(eng.agent_pos), d["pos0"])
    for k in range(T):
        eng.step(torch.from_numpy(d["actions"][k]).cuda(), turn=k + 1)
        for key, mine in (("grid", eng.grid), ("pos", eng.agent_pos), ("obs", eng.obs), ("rewards", eng.rewards), ("total_reward", eng.total_reward)):
            assert np.array_equal(_np(mine), d[key][k]), f"{name}: {key} differs from the reference at turn {k + 1}"
        assert np.array_equal(I.fold_kinds(_np(eng.target_types)), d["target_kinds"][k]), f"{name}: target kinds differ at turn {k + 1}"
        assert np.array_equal(_np(eng.target_types), exp["target_types"][k])
    # ... and with the engine's own action draws (the counter model's)
    eng2 = _bound(ws, E)
    for k in range(T):
        eng2.step(random_actions=True, turn=k + 1)
        assert np.array_equal(_np(eng2.actions), d["actions"][k]) and np.array_equal(_np(eng2.rewards), d["rewards"][k])
    assert np.array_equal(_np(eng2.total_reward), d["total_reward"][-1]) and np.array_equal(_np(eng2.grid), d["grid"][-1])


# ---------------------------------------------------------------------------------------------------------------- 5
FAMILIES = [
    # name, spec, envs, options, (family, lanes, specialised), kernel name prefix
    ("step_fast specialised", lambda: I.iowa_spec(20, 20, 2, 2, 0.01, 21), 4096, {}, (N.FAMILY_WAVE, 64, 1), "step_fast<true, 2, 8, 2, 20, 20"),
    ("step_fast prebuilt", lambda: I.iowa_spec(20, 20, 2, 2, 0.01, 22), 4096, {"jit": 0}, (N.FAMILY_WAVE, 64, 0), "step_fast<true, 0, 0, 0, 0, 0"),
    ("step_big", lambda: I.iowa_spec(72, 72, 2, 2, 0.01, 23, direct=True), 256, {}, (N.FAMILY_WORKGROUP, 256, 1), "step_big<"),
    ("step_big prebuilt", lambda: I.iowa_spec(72, 72, 2, 2, 0.01, 24, direct=True), 256, {"jit": 0}, (N.FAMILY_WORKGROUP, 256, 0), "step_big<"),
    ("generic, a workgroup per env", lambda: I.iowa_spec(72, 72, 2, 2, 0.01, 25), 256, {"force_generic": 1}, (N.FAMILY_GENERIC, 256, 1), "step_kernel<256"),
    ("generic, a wave per env", lambda: I.iowa_spec(9, 9, 2, 2, 0.10, 26), 64, {"force_generic": 1}, (N.FAMILY_GENERIC, 64, 1), "step_kernel<64"),
    ("generic, packed", lambda: I.iowa_spec(20, 20, 2, 2, 0.01, 27, direct=True), 4096, {}, (N.FAMILY_GENERIC, 32, 1), "step_kernel<32"),
]


@pytest.mark.parametrize("case", FAMILIES, ids=[c[0] for c in FAMILIES])
def test_every_kernel_family(torch_cuda, case):
    """A batch that reaches each kernel family (the plan says which, and is asserted), device-drawn actions and given ones, all envs against the
    checker; both outcomes of every deck must occur, and (worlds with the twins) a deck stepped on in the turn it was spawned."""
    torch = torch_cuda
    name, make, E, opts, (family, lanes, specialised), prefix = case
    ws = make()
    T1, T2 = 12, 12
    if ws.height >= 72:
        ws.spawn_prob[1] = 0.02            # (two agents on 4 900 cells: enough decks to meet within the turns played)
    with N.options(**opts):
        plan = N.plan(ws.to_config(E, 0))
        assert (plan["family"], plan["lanes_per_env"], plan["specialised"]) == (family, lanes, specialised), plan
        assert plan["kernel"].startswith(prefix), plan["kernel"]
        eng = _bound(ws, E)
    info = eng.launch_info()
    assert f"specialised={specialised}" in info, info
    given = _given_actions(ws, E, T2, seed=E + T2)
    first = I.expected_run(ws, E, T1)
    last = first["grid"][-1], first["pos"][-1], first["total_reward"][-1]
    second = I.expected_run(ws, E, T2, actions=given, first_turn=T1 + 1, start=last)
    for k in range(T1):
        eng.step(random_actions=True, turn=k + 1)
        _assert_turn(eng, first, k, name)
    for k in range(T2):
        eng.step(torch.from_numpy(given[k]).cuda(), turn=T1 + 1 + k)
        _assert_turn(eng, second, k, name + " (given actions)")
    both = dict(target_types=np.concatenate([first["target_types"], second["target_types"]]), rewards=np.concatenate([first["rewards"], second["rewards"]]))
    cov = I.coverage(both)
    assert all(plain >= 1 and loss >= 1 for plain, loss in cov["pairs"].values()), cov
    assert (second["target_types"] == I.NO_TARGET).any()
    if ws.type_rule[I.FRESH0]:
        assert cov["fresh"] >= 1, cov


# ---------------------------------------------------------------------------------------------------------------- 6
ENTRY_WORLDS = [("fast", lambda: I.iowa_spec(12, 10, 3, 2, 0.08, 31), 96), ("generic", lambda: I.iowa_spec(9, 9, 2, 2, 0.10, 32), 64),
                ("big", lambda: I.iowa_spec(72, 72, 3, 2, 0.03, 33, direct=True), 48)]


@pytest.mark.parametrize("case", ENTRY_WORLDS, ids=[c[0] for c in ENTRY_WORLDS])
def test_rollout_in_one_launch_and_as_a_loop(torch_cuda, case):
    torch = torch_cuda
    _name, make, E = case
    ws = make()
    T = 16
    given = _given_actions(ws, E, T, seed=5, bad=0.0)
    exp = I.expected_run(ws, E, T, actions=given)
    for write_obs in (True, False):             # with observations: the turn loop inside one launch where the plan has it; without: a loop of launches
        eng = _bound(ws, E)
        rew = torch.zeros((T, E, ws.num_agents), dtype=torch.float32, device="cuda:0")
        eng.rollout(T, actions=torch.from_numpy(given).cuda(), rewards_out=rew, write_obs=write_obs)
        assert np.array_equal(_np(rew), exp["rewards"])
        assert np.array_equal(_np(eng.total_reward), exp["total_reward"][-1]) and np.array_equal(_np(eng.grid), exp["grid"][-1])
        assert np.array_equal(_np(eng.target_types), exp["target_types"][-1])       # no turn stride of its own: the last turn stays
    free = I.expected_run(ws, E, T)
    eng = _bound(ws, E)
    eng.rollout(T, random_actions=True)
    assert np.array_equal(_np(eng.total_reward), free["total_reward"][-1]) and np.array_equal(_np(eng.target_types), free["target_types"][-1])
    assert np.array_equal(_np(eng.rewards), free["rewards"][-1]) and np.array_equal(_np(eng.grid), free["grid"][-1])


@pytest.mark.parametrize("case", ENTRY_WORLDS, ids=[c[0] for c in ENTRY_WORLDS])
def test_policy_protocol_with_sgw_act(torch_cuda, case):
    """The sweep + every window once, then sgw_act per agent: sgw_act has no turn argument, the device's turn state (turn_set) says which
    turn's values are drawn.  Also agent after agent through sgw_step (a phase kernel per agent), which carries its turn."""
    torch = torch_cuda
    _name, make, E = case
    ws = make()
    T, A = 14, ws.num_agents
    given = _given_actions(ws, E, T, seed=6)
    exp = I.expected_run(ws, E, T, actions=given)
    eng = _bound(ws, E)
    n_win = int(np.prod(ws.obs_shape[1:]))
    dests = [torch.zeros((E, n_win), device="cuda:0") for _ in range(A)]
    rows = eng.window_rows(dests) if eng.capabilities() & N.CAP_OBSERVE_ROWS else eng.window_rows(None)
    own_rows = bool(eng.capabilities() & N.CAP_OBSERVE_ROWS)
    assert not (eng.capabilities() & N.CAP_RESOLVE)          # a world with a drawn value takes the sequential turn
    for k in range(T):
        turn = k + 1
        eng.turn_set(0, turn - 1)
        acts = torch.from_numpy(given[k]).cuda()
        if own_rows and eng.capabilities() & N.CAP_SWEEP_ROWS:
            eng.sweep_observe_rows(rows, sweep=True, turn=turn)
        elif own_rows:
            eng.step(sweep=True, agent_begin=0, agent_end=0, write_obs=False, turn=turn)
            eng.observe_rows(rows)
        else:
            eng.step(sweep=True, no_move=True, turn=turn)
        seen_tt = torch.full((E, A), 77, dtype=torch.uint8, device="cuda:0")
        for a in range(A):
            window = dests[a].view(E, *ws.obs_shape[1:]) if own_rows else eng.obs[:, a]
            assert np.array_equal(_np(window), exp["obs"][k][:, a]), f"window of agent {a} at turn {turn}"
            eng.act(a, rows, action=acts[:, a].to(torch.int64).contiguous())
            seen_tt[:, a] = eng.target_types[:, a]
        _assert_turn(eng, exp, k, "sgw_act", obs=False)
    # agent after agent through sgw_step
    eng2 = _bound(ws, E)
    for k in range(T):
        acts = torch.from_numpy(given[k]).cuda()
        eng2.step(sweep=True, agent_begin=0, agent_end=0, write_obs=False, turn=k + 1)
        for a in range(A):
            eng2.step(acts, sweep=False, write_obs=False, agent_begin=a, agent_end=a + 1, turn=k + 1)
        _assert_turn(eng2, exp, k, "per-agent sgw_step", obs=False)


def _iowa_env(torch, E, h=20, w=20, a=2, sp=0.05, seed=5, max_turns=30, memory=8):
    from sorrel_amd.examples.iowa.entities import EmptyEntity
    from sorrel_amd.examples.iowa.env import GamblingEnv
    from sorrel_amd.examples.iowa.main import make_config
    from sorrel_amd.examples.iowa.world import GamblingWorld
    from sorrel_amd.models import BaseModel

    class Policy(BaseModel):
        """A fixed linear layer + argmax: deterministic, capturable (no host synchronisation)."""

        def __init__(self, input_size, action_space):
            super().__init__(input_size, action_space, memory_size=memory, num_envs=E, device="cuda:0")
            n = int(np.prod(input_size))
            g = torch.Generator().manual_seed(4321 + n)
            self.weight = torch.randn((n, action_space), generator=g).cuda()

        def take_action(self, state):
            return (state.reshape(state.shape[0], -1) @ self.weight).argmax(dim=1)

    cfg = make_config(h, w, a, 2, spawn_prob=sp, epochs=1, max_turns=max_turns)
    return GamblingEnv(GamblingWorld(cfg, EmptyEntity(), num_envs=E, device="cuda:0", seed=seed), cfg, model_factory=Policy)


def _kind_of_type(env):
    from sorrel_amd.examples.iowa.entities import DECK_KINDS

    out = np.full(256, -1, np.int64)
    for t, p in enumerate(env.world.registry.prototypes):
        if p.kind in DECK_KINDS:
            out[t] = DECK_KINDS.index(p.kind)
    return out


def _expected_encounters(env, tts):
    """int64 [E, A, 4] from per-turn target types [T, E, A] of the example's own type numbering."""
    kinds = _kind_of_type(env)[np.asarray(tts, dtype=np.int64)]
    return np.stack([(kinds == d).sum(axis=0) for d in range(4)], axis=-1)


def _play_and_check(torch, env, turns, what):
    """``turns`` take_turns of ``env`` from where it stands; rewards, totals, target types and the encounters so far against the checker fed
    with the actions the policies took."""
    ws = env.compile_spec()
    E = env.num_envs
    eng = env._ensure_engine()
    start = _np(eng.grid), _np(eng.agent_pos), _np(eng.total_reward)
    enc0 = _np(env.encounters).copy()
    first_turn = env.turn + 1
    acts, rews, tts = [], [], []
    for _ in range(turns):
        env.take_turn()
        acts.append(_np(env.actions)); rews.append(_np(env.rewards)); tts.append(_np(env.target_types))
    exp = I.expected_run(ws, E, turns, epoch=env.epoch, actions=np.stack(acts), first_turn=first_turn, start=start, want_obs=False)
    assert np.array_equal(np.stack(rews), exp["rewards"]), what
    assert np.array_equal(np.stack(tts), exp["target_types"]), what
    assert np.array_equal(_np(env.world.total_reward), exp["total_reward"][-1]) and np.array_equal(_np(eng.grid), exp["grid"][-1]), what
    assert np.array_equal(_np(env.encounters) - enc0, _expected_encounters(env, exp["target_types"])), what
    return exp


def test_recorded_turn_of_the_example(torch_cuda):
    """capture_turn() as Treasurehunt does it: the replayed graph (acts keyed by the device's own turn count, the encounter count recorded
    with the turn) against the checker, and against the same env played eagerly."""
    torch = torch_cuda
    E = 64
    eager, rec = _iowa_env(torch, E), _iowa_env(torch, E)
    assert eager.turn_plan()["loop"] in ("fast", "generic")
    cap = rec.capture_turn(warmup=2)
    assert cap is not None, getattr(rec, "capture_error", None)
    assert rec.turn == 2 and rec.turn_plan()["loop"] == "recorded"
    for _ in range(2):
        eager.take_turn()
    assert np.array_equal(_np(eager.world.total_reward), _np(rec.world.total_reward)) and np.array_equal(_np(eager.encounters), _np(rec.encounters))
    exp = _play_and_check(torch, rec, 20, "recorded")
    _play_and_check(torch, eager, 20, "eager")
    assert cap.turns_replayed == 20
    assert np.array_equal(_np(eager.world.total_reward), _np(rec.world.total_reward)) and np.array_equal(_np(eager.encounters), _np(rec.encounters))
    assert (_kind_of_type(rec)[exp["target_types"].astype(np.int64)] >= 0).sum() > 0
    rec.reset()                                     # the device's turn state follows the host's into the next epoch
    assert int(_np(rec.encounters).sum()) == 0
    _play_and_check(torch, rec, 6, "recorded, next epoch")


def test_speculative_turn_falls_back(torch_cuda):
    """No SGW_CAP_RESOLVE for a world with a drawn value: a speculative environment plays the same turns as the eager one."""
    torch = torch_cuda
    E = 64
    env = _iowa_env(torch, E, a=3, seed=9)
    env.speculate_turns = "always"
    assert not (env._ensure_engine().capabilities() & N.CAP_RESOLVE)
    _play_and_check(torch, env, 12, "speculate_turns = always")
    # ... and where the capability IS advertised (no drawn value) the commit of sgw_turn_resolve keeps the record
    from sorrel_amd.spec import treasurehunt_spec
    ws = treasurehunt_spec(16, 16, 4, 2, spawn_prob=0.1, seed=3)
    ref, spec_eng = _bound(ws, 32), _bound(ws, 32)
    assert spec_eng.capabilities() & N.CAP_RESOLVE
    for k in range(6):
        ref.step(random_actions=True, turn=k + 1)
        spec_eng.step(sweep=True, agent_begin=0, agent_end=0, write_obs=False, turn=k + 1)
        rows = spec_eng.speculation_windows(None)
        acts = ref.actions.t().contiguous().view(-1).to(torch.int64)      # agent-major, as the rows are
        spec_eng.turn_resolve(1, rows, acts)
        p = 1
        while spec_eng.spec_count(p):               # (these actions do not depend on the windows: a dirty row gets the same one again)
            idx = spec_eng.spec_dirty(p)
            p += 1
            assert p <= ws.num_agents + 1
            spec_eng.turn_resolve(p, rows, acts[idx].contiguous())
        for name in ("grid", "agent_pos", "rewards", "total_reward", "target_types"):
            assert np.array_equal(_np(getattr(ref, name)), _np(getattr(spec_eng, name))), (name, k)


# ---------------------------------------------------------------------------------------------------------------- 7
def test_environment_two_epochs(torch_cuda):
    torch = torch_cuda
    env = _iowa_env(torch, 64, sp=0.03, max_turns=25)
    seen = []

    class Log:
        def record_turn(self, epoch, loss, reward, epsilon, encounters=None):
            seen.append((epoch, reward, encounters))

    for epoch in range(2):
        env.reset()
        assert int(_np(env.encounters).sum()) == 0 and all(int(_np(a.encounters).sum()) == 0 for a in env.agents)
        exp = _play_and_check(torch, env, 25, f"epoch {epoch}")
        assert int(_np(env.encounters).sum()) > 0
        assert np.array_equal(_np(env.agents[1].encounters), _np(env.encounters)[:, 1])
        assert env.agents[0].encounter_counts() == {k: int(v) for k, v in zip(I.DECK_KINDS, _np(env.encounters)[:, 0].sum(axis=0))}
        assert np.array_equal(_np(env.world.total_reward), exp["total_reward"][-1])
    env.reset()
    assert int(_np(env.encounters).sum()) == 0
    # the example's epoch loop: the encounters of the epoch in every record
    env2 = _iowa_env(torch, 32, sp=0.05, max_turns=12)
    hist = env2.run_experiment(logger=Log(), epochs=1, max_turns=12)
    assert len(hist) == 2 and len(seen) == 2
    for m, (_e, reward, enc) in zip(hist, seen):
        assert enc == m["encounters"] and set(enc) == set(I.DECK_KINDS) and reward == m["mean_total_reward"]
    assert hist[-1]["encounters"] == env2.encounter_counts() and sum(hist[-1]["encounters"].values()) > 0
    # device-random agents: the same bookkeeping through the fused turn
    from sorrel_amd.examples.iowa.entities import EmptyEntity
    from sorrel_amd.examples.iowa.env import GamblingEnv
    from sorrel_amd.examples.iowa.main import make_config
    from sorrel_amd.examples.iowa.world import GamblingWorld
    cfg = make_config(spawn_prob=0.05, epochs=0, max_turns=20)
    env3 = GamblingEnv(GamblingWorld(cfg, EmptyEntity(), num_envs=128, device="cuda:0", seed=2), cfg)
    assert env3.turn_plan()["loop"] == "fused"
    _play_and_check(torch, env3, 20, "device-random")


# ---------------------------------------------------------------------------------------------------------------- 8
def test_guard_bytes_and_unbound_record(torch_cuda):
    torch = torch_cuda
    ws = I.iowa_spec(12, 10, 3, 2, 0.08, 41)
    E, A, G = 50, 3, 64
    tt_buf = torch.full((G + E * A + G,), 0xA5, dtype=torch.uint8, device="cuda:0")
    rw_buf = torch.full((G + E * A + G,), -123.0, dtype=torch.float32, device="cuda:0")
    eng = make_engine(ws, E, tensors=dict(rewards=rw_buf[G:G + E * A].view(E, A), target_types=tt_buf[G:G + E * A].view(E, A)))
    assert eng.target_types.data_ptr() == tt_buf.data_ptr() + G
    eng.reset(epoch=0)
    exp = I.expected_run(ws, E, 10)
    n_win = int(np.prod(ws.obs_shape[1:]))
    rows = eng.window_rows([torch.zeros((E, n_win), device="cuda:0") for _ in range(A)])
    for k in range(10):
        if k % 2 == 0:
            eng.step(random_actions=True, turn=k + 1)
        else:                                              # the same turn through sgw_act
            acts = torch.from_numpy(exp["actions"][k]).cuda()
            eng.turn_set(0, k)
            eng.step(sweep=True, agent_begin=0, agent_end=0, write_obs=False, turn=k + 1)
            for a in range(A):
                eng.act(a, None, action=acts[:, a].to(torch.int64).contiguous())
        assert np.array_equal(_np(eng.target_types), exp["target_types"][k]) and np.array_equal(_np(eng.rewards), exp["rewards"][k])
    eng.rollout(3, random_actions=True)
    for buf, fill in ((tt_buf, 0xA5), (rw_buf, -123.0)):
        assert bool((buf[:G] == fill).all()) and bool((buf[G + E * A:] == fill).all())
    # unbound: nothing is written any more
    eng.bind_target_types(None)
    assert eng.target_types is None
    tt_buf.fill_(0x5A)
    eng.step(random_actions=True)
    eng.rollout(2, random_actions=True)
    eng.turn_set(0, eng.turn)
    eng.step(sweep=True, agent_begin=0, agent_end=0, write_obs=False, turn=eng.turn + 1)
    eng.act(0, None, action=torch.zeros((E,), dtype=torch.int64, device="cuda:0"))
    torch.cuda.synchronize()
    assert bool((tt_buf == 0x5A).all())
    # the record is the plain movers': a Tag engine refuses the binding
    from tests.gpu_common import _tag_spec
    tag = make_engine(_tag_spec(11, 11, 5, 4), 8)
    with pytest.raises(ValueError, match="SGW_AGENT_RULE_MOVE"):
        tag.bind_target_types(True)
