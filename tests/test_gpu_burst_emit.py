"""burst_emit (common.h) -- staged bytes leaving as line-aligned streaming stores with a scalar trip count, a scalar base and peeled, masked
first and last iterations -- behind its four callers: step_fast's whole-env burst (f32 and u8), emit_chunk's interior, fast_rows_emit's
16-byte path; and the two instances of the agent loop's window (the one for launches that stage whole envs, the general one) on one
engine.  Every tensor against the C oracle, turn by turn; what lies around the observations must stay as it was."""
import numpy as np
import pytest

from sorrel_amd import _native as N
from tests import helpers as H
from tests.gpu_common import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu

ALL = ("grid", "pos", "actions", "obs", "rewards", "total")
STATE = ("grid", "pos", "actions", "rewards", "total")


def _th(h, w, a, r, seed=41, spawn_prob=0.01):
    from sorrel_amd.spec import treasurehunt_spec

    return treasurehunt_spec(h, w, a, r, spawn_prob=spawn_prob, seed=seed, dense_prob=0.1)


def _pair(ws, E, first=3, **kw):
    N.set_option("group", 64)          # (small worlds stay on the wave-per-env kernel)
    eng, co = make_engine(ws, E, first=first, **kw), H.COracle(ws, E, first_env_id=first)
    eng.reset(1)
    co.reset(1)
    return eng, co, eng.launch_info()


def _staged(info):
    return int(info.split("obs_stage=")[1].split()[0])


def _whole_turns(eng, co, turns, what=ALL, ctx=""):
    st = 0
    for t in range(1, turns + 1):
        eng.obs.fill_(-7)
        eng.step(random_actions=True, turn=t, advance_turn=False)
        st |= co.step(1, t, random_actions=True)
        assert_same(eng, co, what, ctx=f"{ctx} turn {t}")
    assert eng.status() == st, (ctx, st)


# ------------------------------------------------------------------ 1. every line offset and the ragged end
@pytest.mark.parametrize("agents", [2, 6, 8])
def test_every_line_offset_and_the_ragged_end(torch_cuda, agents):
    """32x32x2, six channels, radius 3: an env's block is 147 float4 per two agents -- an odd number of 16-byte units for 2 and 6 agents, a
    whole number of half lines for 8 (the headline) -- so the blocks of consecutive envs start at every offset within a 128-byte line."""
    ws = _th(32, 32, agents, 3)
    eng, co, info = _pair(ws, 17)
    assert "step_fast<true, 2, 6, 3, 32, 32" in info and _staged(info) > 0, info
    assert int(np.prod(ws.obs_shape)) == 147 * 4 * agents // 2
    _whole_turns(eng, co, 12, ctx=f"{agents} agents")


# ------------------------------------------------------------------ 2. a burst that is first and last iteration at once
def test_a_burst_that_is_first_and_last_iteration_at_once(torch_cuda):
    """16x16x2, radius 1, 2 agents: 27 float4 per env -- one wave-wide store, masked at both ends."""
    ws = _th(16, 16, 2, 1, seed=42)
    eng, co, info = _pair(ws, 19)
    assert int(np.prod(ws.obs_shape)) == 27 * 4
    if _staged(info) <= 0:
        pytest.fail(f"the shape does not stage whole envs ({info}): no burst to test")
    _whole_turns(eng, co, 12, ctx="16x16 r1")


# ------------------------------------------------------------------ 3. guards
@pytest.mark.parametrize("agents", [2, 8])
def test_guards_around_a_view_at_every_16_byte_offset(torch_cuda, agents):
    """The observations go to a contiguous view carved out of a larger buffer, 0, 16, ... 112 bytes behind a 128-byte line, with 64 guard floats
    on either side: the peeled first iteration's idle low lanes and the last one's ragged end write nothing outside the view."""
    torch = torch_cuda
    ws = _th(32, 32, agents, 3, seed=43)
    E = 17
    eng, co, info = _pair(ws, E)
    assert _staged(info) > 0, info
    n = E * int(np.prod(ws.obs_shape))
    buf = torch.empty((64 + 32 + n + 64,), dtype=torch.float32, device="cuda:0")
    assert buf.data_ptr() % 128 == 0
    t, st = 0, 0
    for k in range(8):
        lo = 64 + 4 * k
        view = buf[lo:lo + n].view((E,) + tuple(ws.obs_shape))
        assert view.data_ptr() % 128 == 16 * k and view.is_contiguous()
        for _ in range(5):
            t += 1
            buf.fill_(-9.0)
            eng.step(random_actions=True, turn=t, advance_turn=False, obs_out=view)
            st |= co.step(1, t, random_actions=True)
            torch.cuda.synchronize()
            assert bool((buf[:lo] == -9.0).all()) and bool((buf[lo + n:] == -9.0).all()), (agents, k, t, "guards")
            assert np.array_equal(view.cpu().numpy(), co.obs), (agents, k, t, "view vs the oracle")
            assert_same(eng, co, STATE, ctx=f"{agents} agents offset {16 * k} turn {t}")
    assert eng.status() == st


# ------------------------------------------------------------------ 4. the other emitters
def test_emit_chunk_on_a_run_time_21x21_map(torch_cuda):
    """Treasurehunt 21x21, 2 agents, radius 2, on the prebuilt run-time-map instance: chunks of agents through emit_chunk."""
    N.set_option("jit", 0)
    ws = _th(21, 21, 2, 2, seed=44, spawn_prob=0.03)
    eng, co, info = _pair(ws, 33)
    assert "step_fast<" in info and "specialised=0" in info and int(info.split("stage_agents=")[1].split()[0]) > 0, info
    _whole_turns(eng, co, 10, ctx="21x21 chunks")


def test_u8_observations_at_the_headline_shape(torch_cuda):
    torch = torch_cuda
    ws = _th(32, 32, 8, 3, seed=45)
    eng, co, info = _pair(ws, 9, obs_dtype=torch.uint8)
    assert "step_fast<true, 2, 6, 3, 32, 32" in info and _staged(info) > 0, info
    st = 0
    for t in range(1, 11):
        eng.obs.fill_(249)
        eng.step(random_actions=True, turn=t, advance_turn=False)
        st |= co.step(1, t, random_actions=True)
        assert_same(eng, co, ALL, ctx=f"u8 turn {t}")
    assert eng.obs.dtype == torch.uint8 and eng.status() == st


@pytest.mark.parametrize("E", [5, 7])
def test_sweep_observe_rows_with_a_partly_filled_last_workgroup(torch_cuda, E):
    """sgw_sweep_observe_rows on 32x32x2 with 8 agents: the last workgroup holds one / three live envs, its waves still write their share
    of the agents' runs (fast_rows_emit's 16-byte path through burst_emit)."""
    torch = torch_cuda
    ws = _th(32, 32, 8, 3, seed=46, spawn_prob=0.02)
    eng, co, info = _pair(ws, E)
    assert eng.capabilities() & N.CAP_SWEEP_ROWS, info
    A, Nw = ws.num_agents, int(np.prod(ws.obs_shape[1:]))
    guard = 64
    bufs = [torch.full((guard + E * Nw + guard,), -9.0, device="cuda:0") for _ in range(A)]
    dests = [b[guard:guard + E * Nw].view(E, Nw) for b in bufs]
    rows = eng.window_rows(dests)
    gen = np.random.default_rng(6)
    st = 0
    for t in range(1, 11):
        for b in bufs:
            b.fill_(-9.0)
        eng.sweep_observe_rows(rows, sweep=True, turn=t)
        st |= co.step(1, t, sweep=True, write_obs=False, a0=0, a1=0)
        co.observe()
        torch.cuda.synchronize()
        if t == 1:
            assert "step_fast_rows" in eng.launch_info().split("sweep_rows=")[1], eng.launch_info()
        assert np.array_equal(eng.grid.cpu().numpy(), co.grid), (E, t, "grid after the sweep")
        for k in range(A):
            assert np.array_equal(dests[k].cpu().numpy(), co.obs[:, k].reshape(E, Nw)), (E, t, k, "window vs the oracle")
            assert bool((bufs[k][:guard] == -9.0).all()) and bool((bufs[k][-guard:] == -9.0).all()), (E, t, k, "guards")
        acts = gen.integers(0, len(ws.action_dy), (E, A)).astype(np.uint8)
        eng.step(torch.from_numpy(acts).cuda(), sweep=False, write_obs=False, turn=t, advance_turn=False)
        st |= co.step(1, t, actions=acts, sweep=False, write_obs=False)
        assert_same(eng, co, STATE, ctx=f"{E} envs turn {t} after the acts")
    assert eng.status() == st


# ------------------------------------------------------------------ 5. both instances of the agent loop's window in one run
def test_both_versions_of_the_agent_loop_in_one_run(torch_cuda):
    """The headline shape: turns as two agent-range launches with given actions (the general window: direct stores) alternate with
    whole turns that draw their actions (the window of the launches that stage whole envs)."""
    torch = torch_cuda
    ws = _th(32, 32, 8, 3, seed=47)
    E = 16
    eng, co, info = _pair(ws, E)
    assert "step_fast<true, 2, 6, 3, 32, 32" in info and _staged(info) > 0, info
    gen = np.random.default_rng(7)
    st = 0
    for t in range(1, 21):
        eng.obs.fill_(-7)
        if t % 2:
            acts = gen.integers(0, len(ws.action_dy), (E, 8)).astype(np.uint8)
            dev = torch.from_numpy(acts).cuda()
            eng.step(dev, agent_begin=0, agent_end=4, turn=t, advance_turn=False)
            eng.step(dev, sweep=False, agent_begin=4, agent_end=8, turn=t, advance_turn=False)
            st |= co.step(1, t, actions=acts, a0=0, a1=4)
            st |= co.step(1, t, actions=acts, sweep=False, a0=4, a1=8)
        else:
            eng.step(random_actions=True, turn=t, advance_turn=False)
            st |= co.step(1, t, random_actions=True)
        assert_same(eng, co, ALL, ctx=f"turn {t} ({'two ranges' if t % 2 else 'whole turn'})")
    assert eng.status() == st
