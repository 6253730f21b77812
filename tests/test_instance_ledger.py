"""The instance ledger on the CPU (tests/instance_ledger.py): every case plans the instance it claims, the cases cover every instance of the
seven turn-kernel templates that libsgw.so holds, nothing listed as unreachable can be named by any plan, and on the C oracle every case's
world does what its instance exists for.  tests/test_gpu_instances.py then launches the cases."""
import itertools

import numpy as np
import pytest

from sorrel_amd import _native as N
from tests import helpers as H
from tests import instance_ledger as L

IDS = [e.id for e in L.ENTRIES]


def _plan(entry, num_envs=None, options=None):
    with N.options(**(entry.options if options is None else options)):
        return N.plan(entry.config(num_envs))


def _named(plan):
    """Every instance a plan names, in any role."""
    out = set()
    for key in ("kernel", "kernel_prebuilt", "kernel_plain", "kernel_rollout", "kernel_walk", "kernel_phase", "kernel_observe_rows"):
        if "<" in plan[key]:
            out.add(H.canonical_instance(plan[key], plan["lanes_per_env"]))
    return out


# ------------------------------------------------------------------ (a) each case plans what it claims
@pytest.mark.parametrize("entry", L.ENTRIES, ids=IDS)
def test_each_case_plans_the_instance_it_claims(built, entry):
    assert entry.options["jit"] == 0 and set(entry.options) - {"jit"} <= set(L.FORCING_OPTIONS)
    plan = _plan(entry)
    assert plan["specialised"] == 0, plan
    key = L.ROLE_KEY[entry.role]
    if key is not None:
        assert "<" in plan[key], (entry.id, key, plan[key])
        assert H.canonical_instance(plan[key], plan["lanes_per_env"]) == entry.instance, (entry.id, key, plan[key])
    if entry.role == "rollout":
        assert plan["rollout_in_one_launch"] == 1
    if entry.role == "walk":      # fewer walking workgroups than envs, and not a divisor of the batch
        assert 0 < plan["walk_blocks"] < entry.num_envs and entry.num_envs % plan["walk_blocks"] and plan["walk_min_envs"] < entry.num_envs <= plan["walk_max_envs"]
    if entry.role == "sweep_rows":      # step_fast_rows: a one-hot wave-per-env engine whose whole env leaves in one staged burst
        assert plan["family"] == N.FAMILY_WAVE and plan["obs_stage"] > 0 and plan["onehot"] == 1 and plan["whole_env_burst"] == 1
    if entry.role == "phase_kernel":    # the byte-gather phase kernel: a workgroup-per-env engine without a phase_rows instance
        assert plan["family"] == N.FAMILY_WORKGROUP and plan["phase_kernel"] == 1 and "phase_rows" not in plan["kernel_phase"]
        assert plan["onehot"] == (1 if entry.instance[1] == ("true",) else 0)
    if entry.role in ("phase_rows", "observe_rows"):
        assert plan["onehot"] == 1


# ------------------------------------------------------------------ (b) completeness
def test_the_ledger_and_the_unreachable_list_are_the_library(built):
    have = {h for h in H.library_instances() if h[0] in L.TEMPLATES}
    ledger = {e.instance for e in L.ENTRIES}
    unreachable = {u[0] for u in L.UNREACHABLE}
    assert not (ledger & unreachable), "an instance is both launched and listed as unreachable"
    missing, gone = have - ledger - unreachable, (ledger | unreachable) - have
    assert not missing, f"instances of libsgw.so without a case in tests/instance_ledger.py: {sorted(missing)}"
    assert not gone, f"the ledger names instances the library does not hold: {sorted(gone)}"
    assert len(IDS) == len(set(IDS))
    by_template = {t: len([h for h in have if h[0] == t]) for t in L.TEMPLATES}
    assert sum(by_template.values()) == len(have) >= 107, by_template


# ------------------------------------------------------------------ (c) UNREACHABLE is a finding, not an escape
def test_no_plan_names_an_unreachable_instance(built):
    """The sweep of sgw_plan: the ledger's worlds x batch sizes {33, 4 096, 16 384, 65 536} x every value of every forcing option (one
    option at a time, then every pair of non-default values), with jit = 0 and with jit = 1 (whose plans name the prebuilt twin).  An
    instance listed in UNREACHABLE may appear in none of them -- and has to quote the line of plan.h that shadows it."""
    import os

    with open(os.path.join(H.ROOT, "sorrel_amd", "csrc", "plan.h")) as fh:
        plan_h = fh.read()
    for inst, line, why in L.UNREACHABLE:
        assert line.strip() and line.strip() in plan_h and why, f"{inst}: quote the shadowing line of plan.h"
    listed = {u[0] for u in L.UNREACHABLE}
    seen, plans = set(), 0
    worlds = {}
    for e in L.ENTRIES:
        worlds.setdefault(e.world, e)
    settings = [{}] + [{k: v} for k, vs in L.FORCING_OPTIONS.items() for v in vs]
    settings += [{k1: v1, k2: v2} for (k1, vs1), (k2, vs2) in itertools.combinations(L.FORCING_OPTIONS.items(), 2) for v1 in vs1[1:] for v2 in vs2[1:]]
    for e in worlds.values():
        for E, jit in itertools.product((33, 4096, 16384, 65536), (0, 1)):
            for more in settings:
                try:
                    plan = _plan(e, E, dict(more, jit=jit))
                except ValueError:      # (a world the LDS-resident path refuses under these options)
                    continue
                plans += 1
                named = _named(plan)
                assert not (named & listed), (e.id, E, more, sorted(named & listed))
                seen |= named
    have = {h for h in H.library_instances() if h[0] in L.TEMPLATES}
    assert plans > 10000
    # (what the sweep reaches by name: everything but the two roles sgw_plan has no field for)
    unnamed = {h for h in have if h[0] == "step_fast_rows"}
    assert have - seen - listed <= unnamed, sorted(have - seen - listed)


# ------------------------------------------------------------------ (d) no case is vacuous
def _trace(entry):
    """The case's T turns on the C oracle, each as sweep-only + the agents (the same draws as the fused turn): what happened."""
    w = entry.built()
    ws = w.spec
    A, H_, W_, r, zA = ws.num_agents, ws.height, ws.width, ws.vision_radius, ws.agent_layer
    co = L.begin_oracle(entry)
    seen = dict(spawned=False, became=False, picked=False, tagged=False, beam=False, turned=False, refused=False, over_edge=False,
                fraction=False, clipped=False, high_moved=False, high_blocked=False, status=0)
    spawners = [t for t in range(ws.num_types) if ws.type_rule[t] == N.RULE_SPAWN and ws.spawn_prob[t] > 0]
    becomers = [t for t in range(ws.num_types) if ws.type_rule[t] == N.RULE_BECOME_IF]
    dy, dx = np.asarray(ws.action_dy), np.asarray(ws.action_dx)
    for t in range(1, entry.turns + 1):
        acts = L.actions_for(entry, t)
        g0, p0, s0, d0 = co.grid.copy(), co.pos.copy(), co.agent_state.copy(), co.agent_dir.copy()
        seen["status"] |= co.step(L.EPOCH, t, sweep=True, write_obs=False, a0=0, a1=0)
        g1 = co.grid.copy()
        changed = g0 != g1
        seen["spawned"] |= bool(np.isin(g0[changed], spawners).any())
        other = np.ones(ws.layers, bool)
        other[zA] = False
        seen["became"] |= bool(np.isin(g0[:, other][changed[:, other]], becomers).any())
        p = p0.astype(np.int64)
        seen["over_edge"] |= bool(((p[..., 0] < r) | (p[..., 0] >= H_ - r) | (p[..., 1] < r) | (p[..., 1] >= W_ - r)).any())
        if acts is None:
            seen["status"] |= co.step(L.EPOCH, t, random_actions=True, sweep=False)
        else:
            seen["status"] |= co.step(L.EPOCH, t, actions=acts, sweep=False)
        a = co.actions.astype(np.int64)
        wants = (dy[a] != 0) | (dx[a] != 0)
        moved = (co.pos != p0).any(axis=2)
        seen["refused"] |= bool((wants & ~moved).any())
        seen["picked"] |= bool((moved & (co.rewards != 0)).any())
        seen["tagged"] |= bool((co.agent_state != s0).any())
        seen["turned"] |= bool((co.agent_dir != d0).any())
        seen["beam"] |= bool((g1[:, other] != co.grid[:, other]).any())
        seen["fraction"] |= bool((co.obs != np.round(co.obs)).any())
        if A > 64:
            seen["high_moved"] |= bool(moved[:, 64:].any())
            seen["high_blocked"] |= bool((wants & ~moved)[:, 64:].any())
    if ws.obs_post == N.OBS_POST_CLIP255_DIV255:      # some cell in an agent's window whose layers add up past 255, seen as exactly 1.0
        co.observe()
        app = np.asarray(ws.appearance, dtype=np.float64)
        sums = app[co.grid.astype(np.int64)].sum(axis=1)                     # [E, H, W, C]
        for e, k in itertools.product(range(entry.num_envs), range(A)):
            y, x = int(co.pos[e, k, 0]), int(co.pos[e, k, 1])
            for c, j, i in zip(*np.nonzero(co.obs[e, k] == 1.0)):
                yy, xx = y + j - r, x + i - r
                if 0 <= yy < H_ and 0 <= xx < W_ and sums[e, yy, xx, c] > 255.0:
                    seen["clipped"] = True
    return seen


@pytest.mark.parametrize("entry", L.ENTRIES, ids=IDS)
def test_no_case_is_vacuous_on_the_oracle(built, entry):
    ws = entry.built().spec
    seen = _trace(entry)
    want = ["over_edge", "refused"]
    if any(ws.type_rule[t] == N.RULE_SPAWN for t in range(ws.num_types)):
        want.append("spawned")
    if ws.agent_rule == N.AGENT_RULE_TAG:
        want.append("tagged")
    else:
        want.append("picked")
    if ws.agent_rule == N.AGENT_RULE_CLEANUP:
        want += ["beam", "turned"]
    if any(ws.type_rule[t] == N.RULE_BECOME_IF for t in range(ws.num_types)):
        want.append("became")
    if entry.instance[1][:1] == ("false",) or (entry.instance[0] == "step_kernel" and entry.instance[1][1] == "false") or entry.instance == ("phase_kernel", ("false",)):
        want.append("fraction")
    if ws.obs_post == N.OBS_POST_CLIP255_DIV255:
        want.append("clipped")
    if ws.num_agents > 64:
        want += ["high_moved", "high_blocked"]
    missing = [k for k in want if not seen[k]]
    assert not missing, f"{entry.id}: in {entry.turns} turns of {entry.num_envs} envs the oracle never saw {missing}"
    assert seen["status"] == 0, "the worlds of the ledger are well-formed: no status bit"
