"""The premise of step_fast's write-back, pinned on the C oracle alone: in a plain mover world a turn changes only the cells in which something
can have spawned (they held the spawning type before the turn) and each agent's old and new cell.  The kernel writes back exactly that set --
the 16-byte units with a spawn hit and the movers' two bytes -- so a turn that changed any other cell would leave a stale byte in the grid."""
import numpy as np
import pytest

from tests import helpers as H
from tests.touched_common import add_events, turn_events

TURNS = 200
ENVS = 12


def _th(h, w, a, seed, spawn_prob):
    from sorrel_amd.spec import treasurehunt_spec

    return treasurehunt_spec(h, w, a, 3, spawn_prob=spawn_prob, seed=seed, dense_prob=0.1)


@pytest.mark.parametrize("given", [False, True], ids=["drawn_actions", "given_actions"])
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("shape", [(32, 32, 8), (16, 32, 4)], ids=["32x32x2_A8", "16x32x2_A4"])
def test_a_turn_changes_only_spawn_cells_and_the_movers_two_cells(shape, seed, given):
    h, w, a = shape
    ws = _th(h, w, a, seed, spawn_prob=(0.005, 0.05, 0.3)[seed - 1])
    co = H.COracle(ws, ENVS, first_env_id=7 * seed)
    co.reset(seed)
    gen = np.random.default_rng(seed)
    total, worst = {}, 0
    for t in range(1, TURNS + 1):
        g0, p0 = co.grid.copy(), co.pos.copy()
        if given:
            st = co.step(seed, t, actions=gen.integers(0, len(ws.action_dy), (ENVS, a)).astype(np.uint8))
        else:
            st = co.step(seed, t, random_actions=True)
        assert st == 0, (t, st)
        ev = turn_events(ws, g0, p0, co.grid, co.pos, co.rewards)
        assert ev["stray"] == 0, f"turn {t}: {ev['stray']} cells changed that no spawn and no mover accounts for"
        add_events(total, ev)
        worst = max(worst, int((g0 != co.grid).reshape(ENVS, -1).sum(axis=1).max()))
    # the run is not vacuous: things spawned, agents moved, agents were refused, movers stood in units that spawned
    assert total["hits"] > 0 and total["movers"] > 0 and total["blocked"] > 0 and total["mover_in_hit_unit"] > 0, total
    print(f"{shape} seed {seed}: {total}, most cells an env changed in one turn: {worst} of {2 * h * w}")
