"""step_fast's shared Philox pass for a turn's rare draws (the agents' actions and the kinds of what spawned in one block), its two-pass
fallback, the records the agent loop writes lane by lane, and the write-back that leaves untouched 1 KiB rounds of the grid where they
are: every tensor against the C oracle, turn by turn, over at least 50 turns per world and launch mode."""
import numpy as np
import pytest

from sorrel_amd import _native as N
from tests import helpers as H
from tests.gpu_common import *  # noqa: F401,F403
from tests.gpu_common import _move_world

pytestmark = pytest.mark.gpu

TURNS = 50
ALL = ("grid", "pos", "actions", "obs", "rewards", "total")


def _th(spawn_prob, seed=31, h=32, w=32, a=8, r=3):
    from sorrel_amd.spec import treasurehunt_spec

    return treasurehunt_spec(h, w, a, r, spawn_prob=spawn_prob, seed=seed, dense_prob=0.1)


def _layers(h, w, layers, a, r, seed, spawn_layers, spawn_prob, border=True, zA=None):
    """A plain-mover world (gpu_common._move_world: six channels, type 0 spawns) in which only the layers of ``spawn_layers`` are filled with
    the spawning type; the others hold an inert type that no rule, spawn or agent ever changes."""
    from sorrel_amd.spec import NO_BORDER

    ws = _move_world(h, w, layers, 6, a, r, seed, zA=zA)
    inert = 5                                               # (a pick-up type of _move_world: passable, never spawned -- spawn_choices are 2, 3, 4)
    ws.layer_fill_type = [0 if z in spawn_layers else inert for z in range(layers)]
    # (the agents' layer always has its walls: the library refuses a world whose agents could walk off the map)
    ws.layer_border_type = [1 if border or z == ws.agent_layer else NO_BORDER for z in range(layers)]
    ws.spawn_prob = [spawn_prob] + [0.0] * (len(ws.spawn_prob) - 1)
    ws.dense_prob = 0.1
    return ws


# name -> (world, envs, what the launch line must say, whether the whole-env staging -- and with it the shared pass -- is there)
WORLDS = {
    # the headline shape: ~5 spawns per env-turn next to 8 action lanes -- the shared pass; its Sand layer is the round the write-back skips
    "c3_64_envs": (lambda: _th(0.005), 64, "step_fast<true, 2, 6, 3, 32, 32"),
    "c3_no_spawns": (lambda: _th(0.0), 64, "step_fast<true, 2, 6, 3, 32, 32"),                 # an empty list: the action lanes alone
    "c3_half_spawn": (lambda: _th(0.5), 64, "step_fast<true, 2, 6, 3, 32, 32"),                # ~400 hits per turn: the two-pass fallback
    "c3_all_spawn": (lambda: _th(1.0), 64, "step_fast<true, 2, 6, 3, 32, 32"),                 # spawn_full: the fallback, every turn
    # a spawning layer 0 without a border under the agents' layer: the cells of lanes 0 .. A-1's units (the env's first bytes = the first rows
    # of layer 0) spawn, so the lanes that draw actions hold hits of their own
    "collide_32x32x2": (lambda: _layers(32, 32, 2, 8, 3, 7, {0, 1}, 0.01, border=False), 64, "step_fast<true, 2, 6, 3, 32, 32"),
    "collide_16x16x2_A12": (lambda: _layers(16, 16, 2, 12, 2, 8, {0, 1}, 0.04, border=False), 70, "step_fast<true, 2, 6, 2, 16, 16"),
    # one layer: its only round holds the agents and is always written
    "one_layer_32x32": (lambda: _layers(32, 32, 1, 6, 3, 9, {0}, 0.01), 64, "step_fast<true, 1, 6, 3, 32, 32"),
    # three layers of one round each: layer 0 never changes (skipped), layer 1 spawns now and then (skipped in some turns, written in others),
    # layer 2 holds the agents (always written)
    "three_layer_inert_floor": (lambda: _layers(32, 32, 3, 8, 3, 10, {1, 2}, 0.0004), 64, "step_fast<true, 3, 6, 3, 32, 32"),
    "three_layer_agents_middle": (lambda: _layers(32, 32, 3, 5, 2, 11, {0}, 0.001, zA=1), 33, "step_fast<true, 3, 6, 2, 32, 32"),
    # ragged: 19 x 23 x 2 = 874 cells, the last unit is part padding and its round is swept as dwords
    "ragged_19x23x2": (lambda: _th(0.03, seed=12, h=19, w=23, a=5, r=3), 37, "step_fast<true, 2, 6, 3, 19, 23"),
    # ragged with full rounds in front: 33 x 35 x 2 = 2 310 cells = two full rounds + 17 units
    "ragged_33x35x2": (lambda: _th(0.01, seed=13, h=33, w=35, a=7, r=2), 21, "step_fast<true, 2, 6, 2, 33, 35"),
}


def _engine(name, **kw):
    make, E, want = WORLDS[name]
    ws = make()
    N.set_option("group", 64)          # (small worlds stay on the wave-per-env kernel)
    eng, co = make_engine(ws, E, first=5, **kw), H.COracle(ws, E, first_env_id=5)
    info = eng.launch_info()
    if want not in info:
        pytest.fail(f"{name}: expected an instance {want}...> with a compile-time shape, got {info}")
    return ws, E, eng, co, info


def bordered(ws):
    """Walls around the agents' layer: no move can leave the map, the status word stays 0."""
    from sorrel_amd.spec import NO_BORDER

    return ws.layer_border_type[ws.agent_layer] != NO_BORDER


def _spawns(before, after, ws):
    """Cells that held the spawning type and hold something else that is not an agent: what the sweep (and nothing else) did."""
    spawner = int(np.flatnonzero(np.asarray(ws.type_rule) != 0)[0])
    return int(((before == spawner) & (after != spawner) & (after != ws.agent_type[0])).sum())


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_whole_turn_launches_vs_oracle(torch_cuda, name):
    """One launch per turn with actions drawn on device: the shared pass where the hit list and the agents fit one wave, else the two passes."""
    torch = torch_cuda
    ws, E, eng, co, info = _engine(name)
    st = 0                              # the oracle's status word over the run: the engine's must be the same
    staged = int(info.split("obs_stage=")[1].split()[0])
    if staged < 256:
        pytest.fail(f"{name}: the launch does not stage whole envs ({info}): the shared pass cannot run")
    overflow = name in ("c3_half_spawn", "c3_all_spawn")
    epoch, turn = 1, 0
    eng.reset(epoch)
    co.reset(epoch)
    A = ws.num_agents
    per_env_turn, overflowed = [], 0
    for k in range(TURNS):
        if overflow and k and k % 5 == 0:      # a fresh map every five turns: its first sweep fills the spawners again (few are left afterwards)
            epoch, turn = epoch + 1, 0
            eng.reset(epoch)
            co.reset(epoch)
        turn += 1
        before = co.grid.copy()
        eng.obs.fill_(-7.0)
        eng.step(random_actions=True)
        st |= co.step(epoch, turn, random_actions=True)
        assert_same(eng, co, ALL, ctx=f"{name} epoch {epoch} turn {turn}")
        per_env_turn.append(_spawns(before, co.grid, ws) / E)
        overflowed += per_env_turn[-1] > 64 - A
    assert eng.status() == st and (st == 0 or not bordered(ws)), (name, st)
    mean = float(np.mean(per_env_turn))
    # the case really is on the side of the fit test (hits + A <= 64) it was written for
    if overflow:
        assert overflowed >= TURNS // 5, (name, per_env_turn)     # (the mean over the envs is above the limit: most envs took the two passes)
    elif name == "c3_no_spawns":
        assert mean == 0.0
    else:
        assert 0.0 < mean and max(per_env_turn) < 64 - A, (name, per_env_turn)


@pytest.mark.parametrize("name", ["c3_64_envs", "collide_16x16x2_A12", "three_layer_inert_floor", "ragged_33x35x2"])
def test_launches_that_do_not_stage_vs_oracle(torch_cuda, name):
    """A turn as two agent-range launches (the sweep with the first agents, then the rest) and whole turns without observations: neither
    stages, both keep the separate action draw and the kind loop; alternating with whole staged turns on the same engine."""
    torch = torch_cuda
    ws, E, eng, co, info = _engine(name)
    st = 0                              # the oracle's status word over the run: the engine's must be the same
    eng.reset(0)
    co.reset(0)
    A = ws.num_agents
    k = A // 2
    for t in range(1, TURNS + 1):
        mode = t % 3
        if mode == 0:
            eng.step(random_actions=True)
            st |= co.step(0, t, random_actions=True)
            what = ALL
        elif mode == 1:
            eng.obs.fill_(-7.0)
            eng.step(random_actions=True, agent_begin=0, agent_end=k, turn=t, advance_turn=False)
            eng.step(random_actions=True, sweep=False, agent_begin=k, agent_end=A, turn=t, advance_turn=False)
            eng.turn = t
            st |= co.step(0, t, random_actions=True, a0=0, a1=k)
            st |= co.step(0, t, random_actions=True, sweep=False, a0=k, a1=A)
            what = ALL
        else:
            eng.step(random_actions=True, write_obs=False)
            st |= co.step(0, t, random_actions=True, write_obs=False)
            what = ("grid", "pos", "actions", "rewards", "total")
        assert_same(eng, co, what, ctx=f"{name} turn {t} mode {mode}")
    assert eng.status() == st and (st == 0 or not bordered(ws)), (name, st)


@pytest.mark.parametrize("name", ["c3_64_envs", "c3_half_spawn", "collide_16x16x2_A12", "three_layer_inert_floor"])
def test_rollout_several_turns_per_launch_vs_oracle(torch_cuda, name):
    """sgw_rollout: launches of 7 turns each (and a last shorter one), every turn's observations, actions and rewards kept and compared."""
    torch = torch_cuda
    ws, E, eng, co, info = _engine(name)
    st = 0                              # the oracle's status word over the run: the engine's must be the same
    eng.reset(2)
    co.reset(2)
    A = ws.num_agents
    t, per = 0, 7
    while t < TURNS + 2:
        n = min(per, TURNS + 2 - t)
        obs = torch.full((n, E) + tuple(ws.obs_shape), -7.0, device="cuda:0")
        acts = torch.zeros((n, E, A), dtype=torch.uint8, device="cuda:0")
        rews = torch.zeros((n, E, A), dtype=torch.float32, device="cuda:0")
        eng.rollout(n, obs_out=obs, actions_out=acts, rewards_out=rews)
        torch.cuda.synchronize()
        for i in range(n):
            t += 1
            st |= co.step(2, t, random_actions=True)
            for key, mine, ref in (("obs", obs[i], co.obs), ("actions", acts[i], co.actions), ("rewards", rews[i], co.rewards)):
                assert np.array_equal(mine.cpu().numpy(), ref), f"{name} turn {t}: {key}"
        assert_same(eng, co, ("grid", "pos", "actions", "rewards", "total"), ctx=f"{name} after turn {t}")
    assert t >= TURNS and eng.status() == st and (st == 0 or not bordered(ws)), (name, st)


@pytest.mark.parametrize("name", ["c3_64_envs", "three_layer_inert_floor", "ragged_19x23x2"])
def test_auto_reset_inside_the_run_vs_oracle(torch_cuda, name):
    """The in-stream reset every 9 turns: the skipped rounds of the write-back hold the NEW epoch's bytes afterwards, whoever wrote them."""
    torch = torch_cuda
    ws, E, eng, co, info = _engine(name)
    st = 0                              # the oracle's status word over the run: the engine's must be the same
    eng.reset(0)
    co.reset(0)
    max_turns = 9
    eng.set_auto_reset(max_turns)
    epoch, turn = 0, 0
    for k in range(TURNS + 6):
        eng.step(random_actions=True)
        turn += 1
        st |= co.step(epoch, turn, random_actions=True)
        assert_same(eng, co, ("obs", "rewards", "actions"), ctx=f"{name} step {k}")
        if turn == max_turns:
            assert np.array_equal(eng.episode_return.cpu().numpy(), co.total), f"{name} step {k}: episode returns"
            epoch, turn = epoch + 1, 0
            co.reset(epoch)
            assert (eng.epoch, eng.turn) == (epoch, 0)
        assert_same(eng, co, ("grid", "pos", "total"), ctx=f"{name} step {k} (epoch {epoch})")
    assert epoch >= 5 and eng.status() == st and (st == 0 or not bordered(ws)), (name, st)


@pytest.mark.parametrize("name", ["c3_64_envs", "collide_32x32x2", "three_layer_inert_floor"])
def test_sweep_only_launch_then_acts_vs_oracle(torch_cuda, name):
    """A policy-driven turn: the sweep and every window in one launch in which nobody acts (the kind loop, the hit units' write-back), then one
    sgw_act per agent; every third turn is a whole fused turn on the same engine."""
    torch = torch_cuda
    ws, E, eng, co, info = _engine(name)
    st = 0                              # the oracle's status word over the run: the engine's must be the same
    if not eng.capabilities() & N.CAP_ACT:
        pytest.fail(f"{name}: no sgw_act for this world ({info})")
    eng.reset(0)
    co.reset(0)
    A = ws.num_agents
    rows = eng.window_rows(None)
    for t in range(1, TURNS + 1):
        st |= co.step(0, t, random_actions=True)
        if t % 3 == 0:
            eng.step(random_actions=True, turn=t, advance_turn=False)
            assert_same(eng, co, ALL, ctx=f"{name} turn {t}")
            continue
        acts = torch.from_numpy(co.actions.copy()).cuda()
        eng.step(acts, sweep=True, no_move=True, turn=t, advance_turn=False)
        seen = torch.zeros_like(eng.obs)
        for a in range(A):
            seen[:, a] = eng.obs[:, a]
            eng.act(a, rows, action=acts[:, a].to(torch.int64).contiguous())
        torch.cuda.synchronize()
        assert np.array_equal(seen.cpu().numpy(), co.obs), f"{name} turn {t}: windows at pov time"
        assert_same(eng, co, ("grid", "pos", "rewards", "total"), ctx=f"{name} policy-driven turn {t}")
    assert eng.status() == st and (st == 0 or not bordered(ws)), (name, st)


def test_prebuilt_instance_without_the_specialiser_vs_oracle(torch_cuda):
    """The library's own headline instance (jit = 0: nothing compiled in-process) on the same turns as the specialised one."""
    torch = torch_cuda
    N.set_option("jit", 0)
    name = "c3_64_envs"
    ws, E, eng, co, info = _engine(name)
    st = 0                              # the oracle's status word over the run: the engine's must be the same
    assert "specialised=0" in info, info
    eng.reset(3)
    co.reset(3)
    for t in range(1, TURNS + 1):
        eng.step(random_actions=True)
        st |= co.step(3, t, random_actions=True)
        assert_same(eng, co, ALL, ctx=f"prebuilt c3 turn {t}")
    assert eng.status() == st and (st == 0 or not bordered(ws)), (name, st)
