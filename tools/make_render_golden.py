"""TEST INFRASTRUCTURE ONLY -- generate ``tests/golden/render/*.npz`` (+ the sprite PNGs the cases use) from the reference's renderer.

Needs the reference checkout (``oracle/ref_loader.py``) and Pillow.  Usage::

    PYTHONDONTWRITEBYTECODE=1 python tools/make_render_golden.py

What runs is the reference's own ``Environment.take_turn`` (through the harness environments of ``oracle/make_golden.py``), and after
every turn its own ``render_sprite`` and ``image_from_array`` (``sorrel/utils/visualization.py:27-176``) on its own world of entity
objects.  Stored, per case: the sprite files' names and their decoded RGBA tiles (decoded the way ``render_sprite`` decodes them), the
tile of every fixture type id, and per frame the cell type ids (the id convention of the step fixtures), agent positions, the action
each agent took in the turn before the frame, Tag's ``it`` state at that act, the name of every agent's current sprite, the per-layer
planes and the pasted frame.  Data only: no reference source text is stored.  The PNGs are copied as they are (images, under 1 KB each).

Cases: Treasurehunt (two layers, two epochs with a ``reset()`` between them; plus windows over every map edge, a window larger than
the map and a 12 x 12 tile size), Tag (a tag happens and the tagged agent keeps its colour until it moves), Cleanup (three layers,
beams with partial alpha)."""
from __future__ import annotations

import os
import shutil
import sys
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import gridstep_oracle as O  # noqa: E402
from oracle import make_golden as MG  # noqa: E402
from oracle import ref_loader  # noqa: E402
from oracle.make_golden import Ctx  # noqa: E402
from tests import helpers as H  # noqa: E402

OUT_DIR = os.path.join(H.GOLDEN_DIR, "render")
SPRITE_DIR = os.path.join(OUT_DIR, "sprites")
LIMIT = 64 * 1024


def sprite_name(path) -> str:
    """``sorrel/examples/tag/assets/hero-g.png`` -> ``tag-hero-g.png``; ``sorrel/agents/assets/hero.png`` -> ``agents-hero.png``."""
    rel = Path(os.path.expanduser(str(path))).resolve().relative_to(Path(ref_loader.REFERENCE_ROOT).resolve() / "sorrel")
    return "-".join(p for p in rel.parts if p not in ("examples", "assets"))


class Tiles:
    """The sprites a case uses: name -> index, the decoded tiles, the files."""

    def __init__(self, tile_size):
        self.tile_size = list(tile_size)
        self.names, self.paths, self.tiles = [], [], []

    def index(self, path) -> int:
        from PIL import Image

        name = sprite_name(path)
        if name not in self.names:
            self.names.append(name)
            self.paths.append(Path(os.path.expanduser(str(path))).resolve())
            self.tiles.append(np.array(Image.open(os.path.expanduser(str(path))).resize(self.tile_size).convert("RGBA")))
        return self.names.index(name)

    def decode(self, tile_size):
        from PIL import Image

        return np.stack([np.array(Image.open(p).resize(list(tile_size)).convert("RGBA")) for p in self.paths])

    def copy_files(self):
        os.makedirs(SPRITE_DIR, exist_ok=True)
        for name, p in zip(self.names, self.paths):
            assert os.path.getsize(p) < 1024, p
            shutil.copyfile(p, os.path.join(SPRITE_DIR, name))


class Recorder:
    """Frames of one reference environment."""

    def __init__(self, R, vis, tiles: Tiles, type_ids, num_types):
        self.R, self.vis, self.tiles, self.type_ids = R, vis, tiles, type_ids
        self.type_tile = np.full((num_types,), -1, np.int32)
        self.rows = []

    def snap(self, env, actions=None, keep_image=True):
        Agent = self.R["agents"].Agent
        world = env.world
        g = self.type_ids(world)
        for (y, x, z), e in np.ndenumerate(world.map):
            if not isinstance(e, Agent):
                t, s = int(g[z, y, x]), self.tiles.index(e.sprite)
                assert self.type_tile[t] in (-1, s), f"type {t} shows two sprites"
                self.type_tile[t] = s
        row = dict(grid=g, pos=np.array([a.location[:2] for a in env.agents], np.uint8),
                   agent_tile=np.array([self.tiles.index(a.sprite) for a in env.agents], np.int32),
                   it=np.array([bool(getattr(a, "it", False)) for a in env.agents]),
                   actions=np.full((len(env.agents),), 255, np.uint8) if actions is None else np.asarray(actions, np.uint8),
                   turn=env.turn)
        if keep_image:
            planes = self.vis.render_sprite(world, tile_size=self.tiles.tile_size)
            row["planes"] = np.stack(planes)
            row["frame"] = np.array(self.vis.image_from_array(planes))
        self.rows.append(row)
        return row

    def arrays(self, image_frames=None):
        rows = self.rows
        keep = [i for i, r in enumerate(rows) if "planes" in r] if image_frames is None else list(image_frames)
        oob = self.tiles.index(_first_wall_sprite(self.last_world))
        tt = np.where(self.type_tile < 0, oob, self.type_tile).astype(np.int32)
        return dict(tile_names=np.array(self.tiles.names), tiles=np.stack(self.tiles.tiles), type_tile=tt, oob_tile=np.array(oob),
                    grid=np.stack([r["grid"] for r in rows]), pos=np.stack([r["pos"] for r in rows]),
                    agent_tile=np.stack([r["agent_tile"] for r in rows]), it=np.stack([r["it"] for r in rows]),
                    actions=np.stack([r["actions"] for r in rows]), turn=np.array([r["turn"] for r in rows]),
                    image_frames=np.array(keep), planes=np.stack([rows[i]["planes"] for i in keep]),
                    frame=np.stack([rows[i]["frame"] for i in keep]))


def _first_wall_sprite(world):
    return world.get_entities_of_kind("Wall")[0].sprite


def hook_take_turn(R, rec: Recorder, keep_image=lambda env: True):
    """Wrap the reference's ``Environment.take_turn``: a frame before the first turn and one after every turn."""
    Environment = R["environment"].Environment
    orig = Environment.take_turn

    def wrapped(self):
        if self.turn == 0:
            rec.snap(self, keep_image=True)
        orig(self)
        acts = [int(a.model.memory.actions[self.turn - 1]) for a in self.agents]
        rec.last_world = self.world
        rec.snap(self, actions=acts, keep_image=keep_image(self))

    Environment.take_turn = wrapped
    return lambda: setattr(Environment, "take_turn", orig)


def save(name, agent_layer, type_names, arrays, **extra):
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, agent_layer=np.array(agent_layer), type_names=np.array(type_names), **arrays, **extra)
    size = os.path.getsize(path)
    print(f"{name}: {size / 1024:.1f} KiB, {arrays['grid'].shape[0]} frames ({len(arrays['image_frames'])} with images), "
          f"{len(arrays['tile_names'])} sprites")
    assert size <= LIMIT, f"{name}: {size} bytes; shrink the case"


# ------------------------------------------------------------------------------------------------------------------- cases
def case_treasurehunt(R, vis):
    from sorrel_amd.spec import treasurehunt_spec

    turns = 3
    spec = H.oracle_spec(treasurehunt_spec(8, 8, 2, 2, spawn_prob=0.15, seed=3))
    tiles = Tiles([16, 16])
    Ctx.seed, Ctx.env, Ctx.epoch, Ctx.turn, Ctx.spec, Ctx.scripted = spec.seed, 0, 0, 0, spec, None
    env, CounterEmpty = MG.make_treasurehunt_env(R, spec, turns)
    rec = Recorder(R, vis, tiles, lambda w: MG.type_ids_treasurehunt(R, w, CounterEmpty), 7)
    undo = hook_take_turn(R, rec)
    epoch_of = []
    try:
        for epoch in (0, 1):
            if epoch:
                Ctx.epoch = epoch
                env.reset()                         # the reference's reset: same agents, fresh world
            for _ in range(turns):
                Ctx.turn = env.turn + 1
                env.take_turn()
            epoch_of += [epoch] * (turns + 1)
    finally:
        undo()
    arrays = rec.arrays()
    assert len(set(arrays["agent_tile"].reshape(-1).tolist())) == 1, "a Treasurehunt agent changed its sprite"
    # windows on the last frame: one over every edge, one larger than the map -- and the 12 x 12 tile size
    world, extra = env.world, {}
    wins = [((0, 3), 2), ((7, 4), 2), ((3, 0), 2), ((4, 7), 2), ((3, 3), 6), ((1, 6), 1)]
    for i, (loc, v) in enumerate(wins):
        planes = vis.render_sprite(world, location=(loc[0], loc[1], 0), vision=v, tile_size=[16, 16])
        extra[f"win{i}_planes"] = np.stack(planes)
        extra[f"win{i}_frame"] = np.array(vis.image_from_array(planes))
    extra["win_loc"] = np.array([w[0] for w in wins], np.int16)
    extra["win_vision"] = np.array([w[1] for w in wins])
    extra["win_at"] = np.array(len(rec.rows) - 1)
    planes12 = vis.render_sprite(world, tile_size=[12, 12])
    extra["tiles12"] = tiles.decode([12, 12])
    extra["t12_planes"], extra["t12_frame"] = np.stack(planes12), np.array(vis.image_from_array(planes12))
    assert not np.array_equal(extra["tiles12"][:, ::1, ::1], tiles.decode([16, 16])[:, :12, :12]), "resize did nothing"
    save("treasurehunt_8x8_two_epochs", 1, ["Sand", "EmptyEntity", "Wall", "Gem", "Bone", "Food", "TreasurehuntAgent"], arrays,
         epoch=np.array(epoch_of), state_at_pov=np.zeros_like(arrays["actions"]), **extra)
    return tiles


def case_tag(R, vis):
    turns = 8
    for seed in range(1, 200):
        spec = MG.tag_spec(7, 7, 3, 2, seed)
        tiles = Tiles([16, 16])
        import sorrel.examples.tag.agents as tag_agents

        def type_ids(world):
            g = np.zeros((1,) + world.map.shape[:2], np.uint8)
            for (y, x, z), e in np.ndenumerate(world.map):
                g[z, y, x] = (2 if e.it else 3) if isinstance(e, tag_agents.TagAgent) else (1 if e.kind == "Wall" else 0)
            return g

        rec = Recorder(R, vis, tiles, type_ids, 4)
        undo = hook_take_turn(R, rec)
        try:
            ref = MG.run_reference_tag(R, spec, [0], turns)
        finally:
            undo()
        arrays = rec.arrays()
        green = np.array([n.endswith("-g.png") for n in arrays["tile_names"]])[arrays["agent_tile"]]      # [F, A]
        # a tag happened, and the tagged agent is shown in its old colour in some frame after it
        stale = arrays["it"][1:] & ~green[1:] & (arrays["it"][1:] != arrays["it"][:-1])
        if stale.any() and green.any():
            break
    else:
        raise RuntimeError("no seed gave a tag whose victim keeps its colour")
    assert np.array_equal(arrays["grid"][1:], ref["grid"][:, 0]) and np.array_equal(arrays["actions"][1:], ref["actions"][:, 0])
    sap = np.concatenate([np.zeros((1, 3), np.uint8), ref["state_at_pov"][:, 0]])
    save("tag_7x7_tagged", 0, ["EmptyEntity", "Wall", "TagAgent:It", "TagAgent:NotIt"], arrays, state_at_pov=sap,
         epoch=np.zeros(len(rec.rows), np.int64), seed=np.array(seed))
    return tiles


def case_cleanup(R, vis):
    turns = 14
    spec = MG.cleanup_spec(10, 9, 2, 2, 7, beam_radius=2, pollution_p=0.05, apple_p=0.05)
    tiles = Tiles([16, 16])
    import sorrel.examples.cleanup.agents as ca

    def type_ids(world):
        g = np.zeros((3,) + world.map.shape[:2], np.uint8)
        for (y, x, z), e in np.ndenumerate(world.map):
            name = type(e).__name__
            if isinstance(e, ca.CleanupAgent):
                t = 11
            elif isinstance(e, ca.CleanBeam):
                t = 7 + (1 if e.turn_counter >= 1 else 0)
            elif isinstance(e, ca.ZapBeam):
                t = 9 + (1 if e.turn_counter >= 1 else 0)
            else:
                t = {"EmptyEntity": 0, "Sand": 1, "Wall": 2, "CounterRiver": 3, "Pollution": 4, "CounterTree": 5, "Apple": 6}[name]
            g[z, y, x] = t
        return g

    def beams(env):
        return any(isinstance(e, ca.Beam) for e in env.world.map[:, :, 2].reshape(-1))

    rec = Recorder(R, vis, tiles, type_ids, 12)
    kept = []

    def keep(env):
        if beams(env) and len(kept) < 3:
            kept.append(env.turn)
            return True
        return False

    undo = hook_take_turn(R, rec, keep)
    try:
        ref = MG.run_reference_cleanup(R, spec, [0], turns, initial_apples=3)
    finally:
        undo()
    arrays = rec.arrays()
    assert len(arrays["image_frames"]) >= 3, "no beams were fired"
    a = arrays["tiles"][..., 3]
    assert ((a > 0) & (a < 255)).any(), "no sprite with partial alpha"
    assert np.array_equal(arrays["grid"][1:], ref["grid"][:, 0]) and np.array_equal(arrays["actions"][1:], ref["actions"][:, 0])
    moved = arrays["agent_tile"][1:] != arrays["agent_tile"][:-1]
    assert moved.any() and not moved[arrays["actions"][1:] >= 4].any(), "Cleanup sprites change on the four moves only"
    save("cleanup_10x9_beams", 1, ["EmptyEntity", "Sand", "Wall", "River", "Pollution", "AppleTree", "Apple", "CleanBeam", "CleanBeam:aged",
                                   "ZapBeam", "ZapBeam:aged", "CleanupAgent"], arrays,
         state_at_pov=np.zeros_like(arrays["actions"]), epoch=np.zeros(len(rec.rows), np.int64), agent_dir=ref["agent_dir"][:, 0])
    return tiles


def main():
    R = MG._import_reference()
    import sorrel.utils.visualization as vis

    for case in (case_treasurehunt, case_tag, case_cleanup):
        case(R, vis).copy_files()


if __name__ == "__main__":
    main()
