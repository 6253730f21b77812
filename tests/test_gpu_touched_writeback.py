"""step_fast's write-back of what a launch touched -- the 16-byte units in which something spawned, then each mover's old and new cell --
on the headline instance and the launch kinds that share its tail: every tensor of every turn against the C oracle, bit for bit.  Each case
also reads from the oracle's host state that the event it is about really occurred (tests/touched_common.py): a vacuous case fails."""
import numpy as np
import pytest

from sorrel_amd import _native as N
from tests import helpers as H
from tests.gpu_common import *  # noqa: F401,F403
from tests.touched_common import add_events, turn_events

pytestmark = pytest.mark.gpu

HEADLINE = "step_fast<true, 2, 6, 3, 32, 32"
TURNS = 40
ALL = ("grid", "pos", "actions", "obs", "rewards", "total")
STATE = ("grid", "pos", "actions", "rewards", "total")


def _th(spawn_prob=0.01, seed=51, h=32, w=32, a=8, r=3):
    from sorrel_amd.spec import treasurehunt_spec

    return treasurehunt_spec(h, w, a, r, spawn_prob=spawn_prob, seed=seed, dense_prob=0.1)


def _pair(ws, E, first=3, want=HEADLINE, **kw):
    N.set_option("group", 64)          # (small worlds stay on the wave-per-env kernel)
    eng, co = make_engine(ws, E, first=first, **kw), H.COracle(ws, E, first_env_id=first)
    eng.reset(1)
    co.reset(1)
    info = eng.launch_info()
    assert want in info, info
    return eng, co, info


def _action(ws, dy, dx):
    return [k for k in range(len(ws.action_dy)) if (ws.action_dy[k], ws.action_dx[k]) == (dy, dx)][0]


def _place(torch, eng, co, ws, cells, free=()):
    """Every env: agent a on cells[a] of the agents' layer (its former cell and the cells of ``free`` hold the default type)."""
    g, p, z = co.grid, co.pos, ws.agent_layer
    for e in range(g.shape[0]):
        g[e, z, p[e, :, 0], p[e, :, 1]] = ws.default_type
    for y, x in free:
        g[:, z, y, x] = ws.default_type
    for a, (y, x) in enumerate(cells):
        g[:, z, y, x] = ws.agent_type[a]
        p[:, a] = (y, x)
    eng.grid.copy_(torch.from_numpy(g))
    eng.agent_pos.copy_(torch.from_numpy(p))


def _play(torch, eng, co, ws, turns=TURNS, given=None, what=ALL, ctx="", epoch=1, status_extra=0, **kw):
    """`turns` whole-turn launches against the oracle; given(t) -> this turn's [E, A] actions, or None to draw them on the device.
    Returns what happened over the run (touched_common.turn_events, summed) and the oracle's status word."""
    total, st = {}, 0
    okw = {k: v for k, v in kw.items() if k in ("sweep", "write_obs")}
    for t in range(1, turns + 1):
        g0, p0 = co.grid.copy(), co.pos.copy()
        if "obs" in what:
            eng.obs.fill_(-7 if eng.obs.dtype.is_floating_point else 249)
        acts = given(t) if given else None
        if acts is None:
            eng.step(random_actions=True, turn=t, advance_turn=False, **kw)
            st |= co.step(epoch, t, random_actions=True, **okw)
        else:
            eng.step(torch.from_numpy(acts).cuda(), turn=t, advance_turn=False, **kw)
            st |= co.step(epoch, t, actions=acts, **okw)
        assert_same(eng, co, what, ctx=f"{ctx} turn {t}")
        add_events(total, turn_events(ws, g0, p0, co.grid, co.pos, co.rewards))
    assert eng.status() == st | status_extra, (ctx, st)
    assert total["stray"] == 0, (ctx, total)
    print(ctx, total)
    return total, st


# ------------------------------------------------------------------ 1. the headline launch
@pytest.mark.parametrize("E", [5, 64, 257])
def test_whole_turns_of_the_headline_instance(torch_cuda, E):
    """5 and 257 envs: the last workgroup holds one env.  Spawns, movers, refused moves and movers inside a unit that spawned all occur."""
    ws = _th()
    eng, co, info = _pair(ws, E)
    ev, st = _play(torch_cuda, eng, co, ws, ctx=f"{E} envs")
    assert st == 0 and min(ev["hits"], ev["movers"], ev["blocked"], ev["mover_in_hit_unit"]) > 0, ev
    assert ev["changed"] < 64 * E * TURNS, ev       # (a turn touches a few dozen of an env's 2 048 cells: what the write-back rests on)


def test_no_spawns_so_no_hit_unit(torch_cuda):
    ws = _th(spawn_prob=0.0)
    eng, co, info = _pair(ws, 9)
    ev, st = _play(torch_cuda, eng, co, ws, ctx="spawn_prob 0")
    assert ev["hits"] == 0 and ev["movers"] > 0 and ev["blocked"] > 0, ev


def test_many_spawns_the_two_pass_fallback_and_agents_on_fresh_spawns(torch_cuda):
    """spawn_prob 0.3: the first turns hold more hits per env than fit the wave next to the eight action lanes (the two-pass fallback), and
    agents step on what has spawned in the same turn: the unit store and the mover's byte store both carry the agent."""
    ws = _th(spawn_prob=0.3)
    eng, co, info = _pair(ws, 9)
    ev, st = _play(torch_cuda, eng, co, ws, ctx="spawn_prob 0.3")
    assert ev["most_hits"] > 64 - ws.num_agents and ev["on_fresh_spawn"] > 0 and ev["mover_in_hit_unit"] > 0, ev


def test_spawn_full(torch_cuda):
    ws = _th(spawn_prob=1.0)
    eng, co, info = _pair(ws, 9)
    ev, st = _play(torch_cuda, eng, co, ws, ctx="spawn_full")
    assert ev["most_hits"] > 500 and ev["movers"] > 0, ev       # (turn 1: every spawning cell of the map)


# ------------------------------------------------------------------ 2. given actions
def test_every_agent_walks_into_the_wall_so_nobody_moves(torch_cuda):
    torch = torch_cuda
    ws = _th(spawn_prob=0.02)
    E = 9
    eng, co, info = _pair(ws, E)
    _place(torch, eng, co, ws, [(1, 2 + 3 * a) for a in range(8)])
    up = np.full((E, 8), _action(ws, -1, 0), np.uint8)
    ev, st = _play(torch, eng, co, ws, given=lambda t: up, ctx="into the wall")
    assert ev["movers"] == 0 and ev["blocked"] == E * 8 * TURNS and ev["hits"] > 0, ev


def test_a_chain_and_two_agents_with_one_target(torch_cuda):
    """Turn 1: agent 0 steps right, agent 1 enters the cell agent 0 has just left (that cell holds an agent before and after: only the ends of
    the chain change); agents 2 and 3 both want (10, 11), the first gets it.  Random given actions from then on."""
    torch = torch_cuda
    ws = _th(spawn_prob=0.02)
    E = 9
    eng, co, info = _pair(ws, E)
    _place(torch, eng, co, ws, [(5, 6), (5, 5), (10, 10), (10, 12), (20, 4), (20, 9), (20, 14), (20, 19)], free=[(5, 7), (10, 11)])
    right, left, down = _action(ws, 0, 1), _action(ws, 0, -1), _action(ws, 1, 0)
    gen = np.random.default_rng(8)
    first = np.tile(np.array([right, right, right, left, down, down, down, down], np.uint8), (E, 1))
    seen = {}

    def given(t):
        if t == 2:      # (the oracle's state after turn 1)
            seen["pos"] = co.pos.copy()
        return first if t == 1 else gen.integers(0, len(ws.action_dy), (E, 8)).astype(np.uint8)

    ev, st = _play(torch, eng, co, ws, given=given, ctx="chain")
    p = seen["pos"]
    assert (p[:, 0] == (5, 7)).all() and (p[:, 1] == (5, 6)).all(), "agent 1 entered the cell agent 0 left"
    assert (p[:, 2] == (10, 11)).all() and (p[:, 3] == (10, 12)).all(), "the first of two agents with one target got it"
    assert ev["hits"] > 0 and ev["mover_in_hit_unit"] > 0, ev


def test_an_invalid_action_index(torch_cuda):
    torch = torch_cuda
    ws = _th()
    E = 9
    eng, co, info = _pair(ws, E)
    gen = np.random.default_rng(9)

    def given(t):
        a = gen.integers(0, len(ws.action_dy), (E, 8)).astype(np.uint8)
        a[t % E, t % 8] = len(ws.action_dy)          # the first index past the table
        a[(t + 3) % E, (t + 5) % 8] = 200
        return a

    ev, st = _play(torch, eng, co, ws, given=given, ctx="invalid actions")
    assert st & N.STATUS_BAD_ACTION and ev["movers"] > 0 and ev["hits"] > 0, (st, ev)


def test_a_bad_position_env(torch_cuda):
    """Agent 0 of one env at (250, 250): the kernel takes it as (0, 0) and says so.  The oracle plays that agent from (0, 0) -- a wall cell in
    the map's corner, from which no move succeeds --; status word (beside SGW_STATUS_BAD_POS) and every tensor must be the oracle's."""
    torch = torch_cuda
    ws = _th()
    E = 9
    eng, co, info = _pair(ws, E)
    eng.agent_pos[E // 2, 0] = 250
    co.pos[E // 2, 0] = 0
    ev, st = _play(torch, eng, co, ws, turns=12, ctx="bad position", status_extra=N.STATUS_BAD_POS)
    assert ev["hits"] > 0 and ev["movers"] > 0 and (co.pos[E // 2, 0] == 0).all(), ev


# ------------------------------------------------------------------ 3. the launch kinds that share the tail
def test_no_move_launch_then_the_acts(torch_cuda):
    """SGW_STEP_NO_MOVE: the sweep and every window in a launch in which nobody acts (hit units only), then the moves without a sweep
    (the movers' bytes only)."""
    torch = torch_cuda
    ws = _th(spawn_prob=0.02)
    E = 9
    eng, co, info = _pair(ws, E)
    gen = np.random.default_rng(10)
    total, st = {}, 0
    for t in range(1, TURNS + 1):
        g0, p0 = co.grid.copy(), co.pos.copy()
        acts = gen.integers(0, len(ws.action_dy), (E, 8)).astype(np.uint8)
        dev = torch.from_numpy(acts).cuda()
        eng.obs.fill_(-7)
        eng.step(dev, sweep=True, no_move=True, turn=t, advance_turn=False)
        st |= co.step(1, t, actions=acts, sweep=True, write_obs=False, a0=0, a1=0)
        co.observe()
        assert_same(eng, co, ("grid", "pos", "obs"), ctx=f"turn {t} after the sweep-only launch")
        assert (co.pos == p0).all()
        eng.step(dev, sweep=False, write_obs=False, turn=t, advance_turn=False)
        st |= co.step(1, t, actions=acts, sweep=False, write_obs=False)
        assert_same(eng, co, STATE, ctx=f"turn {t} after the acts")
        add_events(total, turn_events(ws, g0, p0, co.grid, co.pos, co.rewards))
    assert eng.status() == st == 0
    assert total["stray"] == 0 and min(total["hits"], total["movers"], total["mover_in_hit_unit"]) > 0, total


def test_two_agent_ranges_per_turn(torch_cuda):
    torch = torch_cuda
    ws = _th(spawn_prob=0.02)
    E = 9
    eng, co, info = _pair(ws, E)
    gen = np.random.default_rng(11)
    total, st = {}, 0
    for t in range(1, TURNS + 1):
        g0, p0 = co.grid.copy(), co.pos.copy()
        acts = gen.integers(0, len(ws.action_dy), (E, 8)).astype(np.uint8)
        dev = torch.from_numpy(acts).cuda()
        eng.obs.fill_(-7)
        eng.step(dev, agent_begin=0, agent_end=3, turn=t, advance_turn=False)
        st |= co.step(1, t, actions=acts, a0=0, a1=3)
        assert_same(eng, co, ("grid", "pos", "rewards", "total"), ctx=f"turn {t} after agents 0-2")
        add_events(total, turn_events(ws, g0, p0, co.grid, co.pos, co.rewards, a0=0, a1=3))
        eng.step(dev, sweep=False, agent_begin=3, agent_end=8, turn=t, advance_turn=False)
        st |= co.step(1, t, actions=acts, sweep=False, a0=3, a1=8)
        assert_same(eng, co, ALL, ctx=f"turn {t} after agents 3-7")
    assert eng.status() == st == 0
    assert total["stray"] == 0 and min(total["hits"], total["movers"], total["blocked"], total["mover_in_hit_unit"]) > 0, total


def test_turns_without_a_sweep(torch_cuda):
    ws = _th()
    eng, co, info = _pair(ws, 9)
    ev, st = _play(torch_cuda, eng, co, ws, ctx="sweep=False", sweep=False)
    assert ev["hits"] == 0 and ev["movers"] > 0 and ev["blocked"] > 0, ev


def test_turns_without_observations(torch_cuda):
    ws = _th(spawn_prob=0.02)
    eng, co, info = _pair(ws, 9)
    ev, st = _play(torch_cuda, eng, co, ws, what=STATE, ctx="write_obs=False", write_obs=False)
    assert min(ev["hits"], ev["movers"], ev["mover_in_hit_unit"]) > 0, ev


def test_u8_observations(torch_cuda):
    torch = torch_cuda
    ws = _th(spawn_prob=0.02)
    eng, co, info = _pair(ws, 9, obs_dtype=torch.uint8)
    ev, st = _play(torch, eng, co, ws, ctx="u8")
    assert eng.obs.dtype == torch.uint8 and min(ev["hits"], ev["movers"], ev["mover_in_hit_unit"]) > 0, ev


def test_auto_reset_every_seven_turns(torch_cuda):
    """The in-stream reset rewrites whole grids between launches: the units and bytes a turn does not write hold the NEW epoch's map."""
    ws = _th(spawn_prob=0.02)
    E = 9
    eng, co, info = _pair(ws, E)
    eng.reset(0)
    co.reset(0)
    eng.set_auto_reset(7)
    epoch, turn, total = 0, 0, {}
    for k in range(TURNS):
        g0, p0 = co.grid.copy(), co.pos.copy()
        eng.step(random_actions=True)
        turn += 1
        assert co.step(epoch, turn, random_actions=True) == 0
        assert_same(eng, co, ("obs", "rewards", "actions"), ctx=f"step {k}")
        add_events(total, turn_events(ws, g0, p0, co.grid, co.pos, co.rewards))
        if turn == 7:
            assert np.array_equal(eng.episode_return.cpu().numpy(), co.total), f"step {k}: episode returns"
            epoch, turn = epoch + 1, 0
            co.reset(epoch)
            assert (eng.epoch, eng.turn) == (epoch, 0)
        assert_same(eng, co, ("grid", "pos", "total"), ctx=f"step {k} (epoch {epoch})")
    assert epoch == 5 and eng.status() == 0
    assert total["stray"] == 0 and min(total["hits"], total["movers"], total["mover_in_hit_unit"]) > 0, total


# ------------------------------------------------------------------ 4. other round layouts (kernels specialised in-process)
@pytest.mark.parametrize("shape", [(32, 64, 8), (16, 32, 4)], ids=["2x32x64_four_rounds", "2x16x32_one_round"])
def test_other_round_layouts(torch_cuda, shape):
    """2 x 32 x 64: four 1 KiB rounds, the agents' layer spanning the last two.  2 x 16 x 32: one round that holds both layers."""
    h, w, a = shape
    ws = _th(spawn_prob=0.02, seed=52, h=h, w=w, a=a)
    N.set_option("group", 64)
    probe = make_engine(ws, 9, first=3)
    info = probe.launch_info()
    if "specialised=1" not in info or f"step_fast<true, 2, 6, 3, {h}, {w}" not in info:
        pytest.skip(f"no compile-time-shape instance for {h}x{w}x2 without the in-process specialiser (hipRTC): {info}")
    del probe
    eng, co, info = _pair(ws, 9, want=f"step_fast<true, 2, 6, 3, {h}, {w}")
    ev, st = _play(torch_cuda, eng, co, ws, ctx=f"{h}x{w}x2")
    assert st == 0 and min(ev["hits"], ev["movers"], ev["blocked"], ev["mover_in_hit_unit"]) > 0, ev
