"""What a turn touched in a plain mover world's grid, read from the C oracle's host state: shared by tests/test_touched_cells_cpu.py (the
premise of step_fast's write-back) and tests/test_gpu_touched_writeback.py (whether a case's event really occurred).  Not collected by pytest."""
import numpy as np


def spawner_of(ws):
    return int(np.flatnonzero(np.asarray(ws.type_rule) != 0)[0])


def cell_offsets(ws, pos):
    """[E, A] byte offsets of the agents' cells inside an env (layer-major: the kernel's LDS offsets and RNG indices)."""
    p = pos.astype(np.int64)
    return ws.agent_layer * ws.height * ws.width + p[..., 0] * ws.width + p[..., 1]


def turn_events(ws, g0, p0, g1, p1, rewards=None, a0=0, a1=None):
    """Counts of what happened between (g0, p0) and (g1, p1), one launch or one turn apart; agents [a0, a1) acted.

    stray      changed cells that are neither an acting agent's old or new cell nor held the spawning type before: must be 0
    changed    cells that differ
    hits       cells that held the spawning type and hold one of its spawn choices now
    movers / blocked   acting agents whose position changed / did not
    mover_in_hit_unit  movers whose old or new cell lies in a 16-byte unit in which something spawned
    on_fresh_spawn     movers that entered a cell which held the spawning type before the turn and were rewarded for what they found there
    most_hits          the largest number of hits in one env (add_events keeps the maximum, and sums everything else)
    """
    E = g0.shape[0]
    a1 = ws.num_agents if a1 is None else a1
    f0, f1 = g0.reshape(E, -1), g1.reshape(E, -1)
    sp = spawner_of(ws)
    changed = f0 != f1
    old, new = cell_offsets(ws, p0)[:, a0:a1], cell_offsets(ws, p1)[:, a0:a1]
    allowed = f0 == sp
    np.put_along_axis(allowed, old, True, axis=1)
    np.put_along_axis(allowed, new, True, axis=1)
    hits = (f0 == sp) & np.isin(f1, np.asarray(ws.spawn_choices[sp], dtype=f1.dtype))
    moved = (p0[:, a0:a1] != p1[:, a0:a1]).any(axis=-1)
    pad = (-f0.shape[1]) % 16
    unit_hit = np.pad(hits, ((0, 0), (0, pad))).reshape(E, -1, 16).any(axis=-1)
    in_unit = (np.take_along_axis(unit_hit, old >> 4, axis=1) | np.take_along_axis(unit_hit, new >> 4, axis=1)) & moved
    ev = dict(stray=int((changed & ~allowed).sum()), changed=int(changed.sum()), hits=int(hits.sum()), movers=int(moved.sum()),
              blocked=int((~moved).sum()), mover_in_hit_unit=int(in_unit.sum()), on_fresh_spawn=0,
              most_hits=int(hits.sum(axis=1).max()))       # (the largest number of spawns in one env)
    if rewards is not None:
        ev["on_fresh_spawn"] = int((moved & (np.take_along_axis(f0, new, axis=1) == sp) & (rewards[:, a0:a1] != 0)).sum())
    return ev


def add_events(total, ev):
    for k, v in ev.items():
        total[k] = max(total.get(k, 0), v) if k.startswith("most_") else total.get(k, 0) + v
    return total
