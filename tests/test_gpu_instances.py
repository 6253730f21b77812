"""Every prebuilt instance of the turn kernels in libsgw.so, launched: the cases of tests/instance_ledger.py (one per instance and role, all
with jit = 0), each asserted to launch the instance it names and run against the C oracle bit for bit -- every turn the grid, positions,
actions, observations, rewards, totals and, where the rule keeps them, the agents' types / types at observation time / facings; at the end the
status word.  No tolerance anywhere.  tests/test_instance_ledger.py proves on the CPU that the cases cover the library and are not vacuous.
(The host-selected instances -- act_patch, render_kernel, sample_rows_kernel, turn_resolve, turn_commit_kernel, turn_prev_rows_kernel,
gather_rows_kernel, reset_kernel -- have their own test files and no plan to enumerate them by: they are not in the ledger.)"""
import numpy as np
import pytest

from sorrel_amd import _native as N
from tests import helpers as H
from tests import instance_ledger as L
from tests.gpu_common import *  # noqa: F401,F403
from tests.gpu_common import same_with_agent_state as same

pytestmark = pytest.mark.gpu

STATE = ("grid", "pos", "actions", "rewards", "total")
GUARD = 64      # floats on either side of every per-agent destination
_DEVICE_ERROR = []      # the case whose launch came back with a HIP error: nothing is launched after it


def _begin(torch, entry):
    """The case's engine under the case's options, and the oracle, both at the start of the exercise."""
    for k, v in entry.options.items():
        N.set_option(k, v)          # (process-wide; conftest puts the defaults back after the test)
    w = entry.built()
    E = entry.num_envs
    eng, co = make_engine(w.spec, E, first=L.FIRST_ENV), L.begin_oracle(entry)
    if w.start is None:
        eng.reset(L.EPOCH)
    else:
        g0, p0 = w.start
        eng.epoch = L.EPOCH
        eng.grid.copy_(torch.from_numpy(np.broadcast_to(g0, (E,) + g0.shape).copy()))
        eng.agent_pos.copy_(torch.from_numpy(np.broadcast_to(p0, (E,) + p0.shape).copy()))
        eng.total_reward.zero_()
    same(eng, co, "start", ("grid", "pos", "total"))
    return eng, co


def _launches_the_instance(entry, eng):
    info = eng.launch_info()
    plan = N.plan(eng.config)
    assert "specialised=0" in info and plan["specialised"] == 0, info
    lanes = int(info.split(" group=")[1].split()[0])
    named = {"step": info.split(" group=")[0], "walk": info.split(" group=")[0],
             "phase_rows": info.split(" phase=")[1].split(" big_stage=")[0], "phase_kernel": info.split(" phase=")[1].split(" big_stage=")[0],
             "sweep_rows": info.split(" sweep_rows=")[1]}.get(entry.role)
    if named is None:       # plain / rollout / observe_rows: launch_info does not print them, the plan of this very engine names them
        named = plan[L.ROLE_KEY[entry.role]]
    assert "<" in named and H.canonical_instance(named, lanes) == entry.instance, (entry.id, named, info)
    return plan


def _guarded(torch, E, A, Nw):
    bufs = [torch.full((GUARD + E * Nw + GUARD,), -9.0, device="cuda:0") for _ in range(A)]
    return bufs, [b[GUARD:GUARD + E * Nw].view(E, Nw) for b in bufs]


def _guards_intact(bufs, ctx):
    for k, b in enumerate(bufs):
        assert bool((b[:GUARD] == -9.0).all()) and bool((b[-GUARD:] == -9.0).all()), (ctx, k, "wrote outside the destination")


def _phased_turn(torch, eng, co, entry, t):
    """Sweep-only (+ the first window), then one call per agent: move it, render the next agent's window."""
    ws = entry.built().spec
    A = ws.num_agents
    acts_np = L.actions_for(entry, t)
    acts = torch.from_numpy(acts_np).cuda()
    st = co.step(L.EPOCH, t, actions=acts_np)
    seen, rew = torch.zeros_like(eng.obs), torch.zeros_like(eng.rewards)
    eng.obs.fill_(-7.0)
    eng.step(acts, sweep=True, agent_begin=0, agent_end=0, turn=t, obs_next=True)
    for a in range(A):
        seen[:, a] = eng.obs[:, a]
        # step_launch: `one_phase` (one agent, no sweep, given actions) -> k_rows if usable, else phase_kernel where phase_ok
        eng.step(acts, sweep=False, agent_begin=a, agent_end=a + 1, turn=t, obs_next=a + 1 < A, write_obs=False)
        rew[:, a] = eng.rewards[:, a]
    torch.cuda.synchronize()
    assert np.array_equal(seen.cpu().numpy(), co.obs), f"{entry.id} turn {t}: the windows at pov time"
    assert np.array_equal(rew.cpu().numpy(), co.rewards), f"{entry.id} turn {t}: rewards"
    same(eng, co, f"{entry.id} turn {t}", ("grid", "pos", "actions", "total"))
    return st


@pytest.mark.parametrize("entry", L.ENTRIES, ids=[e.id for e in L.ENTRIES])
def test_prebuilt_instance_vs_the_c_oracle(torch_cuda, entry):
    if _DEVICE_ERROR:
        pytest.fail(f"not launched: the device reported an error in case {_DEVICE_ERROR[0]}")
    try:
        _run_case(torch_cuda, entry)
    except (N.SgwError, RuntimeError):      # (a mismatch is an AssertionError and stops nothing)
        _DEVICE_ERROR.append(entry.id)
        raise


def _run_case(torch, entry):
    eng, co = _begin(torch, entry)
    plan = _launches_the_instance(entry, eng)
    ws = entry.built().spec
    E, A, T, role = entry.num_envs, ws.num_agents, entry.turns, entry.role
    Nw = int(np.prod(ws.obs_shape[1:]))
    st = 0
    if role == "step":
        for t in range(1, T + 1):
            eng.obs.fill_(-7)
            eng.step(random_actions=True, turn=t, advance_turn=False)
            st |= L.oracle_turn(entry, co, t)
            same(eng, co, f"{entry.id} turn {t}")
    elif role == "plain":
        # step_launch: `p.a0 != 0 || p.a1 != p.A` on a staging engine -> k_plain (agent ranges cannot be staged)
        assert plan["stage_agents"] > 0 and A >= 2
        half = A // 2
        for t in range(1, T + 1):
            dev = torch.from_numpy(L.actions_for(entry, t)).cuda()
            eng.obs.fill_(-7)
            eng.step(dev, agent_begin=0, agent_end=half, turn=t, advance_turn=False)
            eng.step(dev, sweep=False, agent_begin=half, agent_end=A, turn=t, advance_turn=False)
            st |= L.oracle_turn(entry, co, t)
            same(eng, co, f"{entry.id} turn {t} (two agent ranges)")
    elif role == "rollout":
        # step_launch: `p.nturns > 1` -> k_multi; sgw_rollout hands all T turns to one launch only where the plan says so
        assert plan["rollout_in_one_launch"] == 1 and (plan["family"] != N.FAMILY_WAVE or plan["obs_stage"] > 0), plan
        eng.turn = 0
        eng.rollout(T)
        for t in range(1, T + 1):
            st |= L.oracle_turn(entry, co, t)
        same(eng, co, f"{entry.id} after sgw_rollout of {T} turns")
    elif role == "walk":
        assert "grid=%d " % plan["walk_blocks"] in eng.launch_info() and plan["walk_blocks"] < E, eng.launch_info()
        for t in range(1, T + 1):
            eng.obs.fill_(-7)
            eng.step(random_actions=True, turn=t, advance_turn=False)
            st |= L.oracle_turn(entry, co, t)
            same(eng, co, f"{entry.id} turn {t}")
        eng.step(sweep=True, agent_begin=0, agent_end=0, write_obs=False, turn=T + 1, advance_turn=False)       # a sweep-only launch walks the batch too
        st |= co.step(L.EPOCH, T + 1, sweep=True, write_obs=False, a0=0, a1=0)
        same(eng, co, f"{entry.id} sweep-only launch", ("grid", "pos", "total"))
    elif role in ("phase_rows", "phase_kernel"):
        for t in range(1, T + 1):
            st |= _phased_turn(torch, eng, co, entry, t)
    elif role in ("observe_rows", "sweep_rows"):
        # sgw_observe_rows launches k_obs_rows itself (observe_rows_impl, not step_launch); sgw_sweep_observe_rows reaches step_launch's
        # `sweep_rows && e->fast` branch -> k_sweep_rows
        assert eng.capabilities() & (N.CAP_OBSERVE_ROWS if role == "observe_rows" else N.CAP_SWEEP_ROWS), eng.launch_info()
        bufs, dests = _guarded(torch, E, A, Nw)
        rows = eng.window_rows(dests)
        for t in range(1, T + 1):
            for b in bufs:
                b.fill_(-9.0)
            if role == "observe_rows":
                eng.step(sweep=True, agent_begin=0, agent_end=0, write_obs=False, turn=t, advance_turn=False)
                eng.observe_rows(rows)
            else:
                eng.sweep_observe_rows(rows, sweep=True, turn=t)
            st |= co.step(L.EPOCH, t, sweep=True, write_obs=False, a0=0, a1=0)
            co.observe()
            torch.cuda.synchronize()
            assert np.array_equal(eng.grid.cpu().numpy(), co.grid), (entry.id, t, "grid after the sweep")
            for k in range(A):
                assert np.array_equal(dests[k].cpu().numpy(), co.obs[:, k].reshape(E, Nw)), (entry.id, t, k, "window vs the oracle")
            _guards_intact(bufs, (entry.id, t))
            acts = L.actions_for(entry, t)
            eng.step(torch.from_numpy(acts).cuda(), sweep=False, write_obs=False, turn=t, advance_turn=False)
            st |= co.step(L.EPOCH, t, actions=acts, sweep=False, write_obs=False)
            same(eng, co, f"{entry.id} turn {t} after the acts", STATE)
    else:
        raise AssertionError(role)
    assert eng.status() == st, (entry.id, st)
