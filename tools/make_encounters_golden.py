"""TEST INFRASTRUCTURE ONLY -- generate ``tests/golden/encounters/cleanup_15x16.npz`` from the reference's Cleanup example.

Needs the reference checkout (``oracle/ref_loader.py``).  Usage::

    PYTHONDONTWRITEBYTECODE=1 python tools/make_encounters_golden.py

Replays the ``cleanup_15x16`` case of ``oracle/make_golden.py`` (same spec, same env ids, 40 turns) through
``make_golden.run_reference_cleanup`` -- the reference's own ``CleanupAgent.act`` -- with ``CleanupAgent`` replaced, for the length of the
run, by a subclass OF THE SAME CLASS NAME (an entity's kind is its class name) that copies ``self.encounters`` after every ``act``.
Stored: the spec, the env ids, the start state, the actions, the kind names and the cumulative counts ``encounters[T, E, A, K]``.  Data
only: no reference source text is stored.  Asserted: the run is the one ``tests/golden/cleanup_15x16.npz`` holds (actions, rewards), every
kind was found at least once, and an act adds exactly one count per layer."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import make_golden as MG  # noqa: E402

NAME, ENV_IDS, TURNS = "cleanup_15x16", [0, 7], 40
OUT_DIR = os.path.join(MG.GOLDEN_DIR, "encounters")


def main() -> int:
    R = MG._import_reference()
    import sorrel.examples.cleanup.agents as ca

    spec = MG.cleanup_spec(15, 16, 4, 3, seed=41, beam_radius=3, pollution_p=0.06, apple_p=0.03)
    kinds = list(MG.CLEANUP_KINDS)
    log = []                                       # one dict per act, in the order the acts happen: env, turn, agent
    Orig = ca.CleanupAgent

    class CleanupAgent(Orig):                      # (the name is the kind the other agents count)
        def act(self, world, action):
            reward = super().act(world, action)
            log.append(dict(self.encounters))
            return reward

    ca.CleanupAgent = CleanupAgent
    try:
        ref = MG.run_reference_cleanup(R, spec, ENV_IDS, TURNS, initial_apples=6)
    finally:
        ca.CleanupAgent = Orig

    E, A, K = len(ENV_IDS), spec.num_agents, len(kinds)
    assert len(log) == E * TURNS * A, (len(log), E, TURNS, A)
    enc = np.zeros((TURNS, E, A, K), dtype=np.int64)
    i = 0
    for e in range(E):
        for t in range(TURNS):
            for a in range(A):
                assert set(log[i]) <= set(kinds), sorted(set(log[i]) - set(kinds))
                enc[t, e, a] = [log[i].get(k, 0) for k in kinds]
                i += 1
    inc = np.diff(np.concatenate([np.zeros((1, E, A, K), np.int64), enc]), axis=0)
    assert (inc >= 0).all() and (inc.sum(axis=-1) == spec.layers).all(), "an act finds one entity per layer"
    assert (enc[-1].sum(axis=(0, 1)) >= 1).all(), dict(zip(kinds, enc[-1].sum(axis=(0, 1)).tolist()))
    assert (inc == 3).any(), "no act found one kind on all three layers"
    old = np.load(os.path.join(MG.GOLDEN_DIR, NAME + ".npz"))
    assert np.array_equal(old["actions"], ref["actions"]) and np.array_equal(old["rewards"], ref["rewards"]), "not the run the step-loop fixture holds"
    assert np.array_equal(old["grid0"], ref["grid0"]) and np.array_equal(old["pos0"], ref["pos0"])
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, NAME + ".npz")
    np.savez_compressed(path, spec_json=np.array(MG.spec_to_json(spec)), env_ids=np.asarray(ENV_IDS, dtype=np.int64), grid0=ref["grid0"],
                        pos0=ref["pos0"], actions=ref["actions"], kinds=np.array(kinds), encounters=enc)
    size = os.path.getsize(path)
    assert size < 100 * 1024, size
    print(f"wrote {path} ({size} bytes); totals: {dict(zip(kinds, enc[-1].sum(axis=(0, 1)).tolist()))}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
