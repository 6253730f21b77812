"""Sprite rendering without a GPU: the integer paste against PIL, the torch path (the CPU product path, and what the kernel is
compared with) against the reference's own pictures (``tests/golden/render``) and against the running reference, the atlas, the
agents' sprite bookkeeping, the reference's module names, and the C ABI's declaration."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from oracle import ref_loader
from sorrel_amd import _native as N
from sorrel_amd.utils import visualization as V
from tests import helpers as H
from tests import render_common as RC


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ------------------------------------------------------------------------------------------------------------- the integers
def test_paste_is_pils_masked_paste_for_every_byte_triple():
    """All 256^3 (dst, src, alpha) triples, on all four bytes (the alpha byte pastes alpha over dst: covered by src == alpha)."""
    from PIL import Image

    a, s, d = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    dst = np.repeat(d.reshape(4096, 4096, 1), 4, axis=2)
    src = np.repeat(s.reshape(4096, 4096, 1), 4, axis=2)
    src[..., 3] = a.reshape(4096, 4096)
    im, top = Image.fromarray(dst, mode="RGBA"), Image.fromarray(src, mode="RGBA")
    im.paste(top, (0, 0), mask=top)
    want = np.array(im)
    got = np.empty_like(want)
    for lo in range(0, 4096, 512):          # (in slabs: the int32 temporaries of the whole table would be 1 GiB)
        got[lo:lo + 512] = V.paste(t(dst[lo:lo + 512]), t(src[lo:lo + 512])).numpy()
    assert np.array_equal(got, want)
    # what the kernel's shortcuts rely on: an opaque pixel replaces, a clear pixel changes nothing
    assert np.array_equal(got[src[..., 3] == 255], src[src[..., 3] == 255]) and np.array_equal(got[src[..., 3] == 0], dst[src[..., 3] == 0])


# ------------------------------------------------------------------------------------------------------------- the fixtures
def test_fixtures_are_present():
    assert RC.FIXTURES == ["cleanup_10x9_beams", "tag_7x7_tagged", "treasurehunt_8x8_two_epochs"]
    for name in RC.FIXTURES:
        assert os.path.getsize(os.path.join(RC.RENDER_DIR, name + ".npz")) <= 64 * 1024


@pytest.mark.parametrize("name", RC.FIXTURES)
def test_torch_path_reproduces_the_reference_pictures(name):
    d = RC.load(name)
    tt = t(RC.type_tile256(d))
    for label, tiles_key, grid, kw, want in RC.cases(d):
        kw = {k: (t(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
        got = V.render_torch(t(grid), t(d[tiles_key]), tt, int(d["oob_tile"]), **kw).numpy()
        assert got.shape == want.shape and got.dtype == np.uint8, (label, got.shape, want.shape)
        assert np.array_equal(got, want), f"{name}: {label} differ"


def test_fixtures_cover_what_they_are_for():
    d = RC.load("tag_7x7_tagged")
    green = np.array([n.endswith("-g.png") for n in d["tile_names"]])[d["agent_tile"]]
    assert (d["it"][1:] != d["it"][:-1]).any(), "no tag happened"
    assert (d["it"] & ~green)[1:].any(), "no tagged agent is shown in its old colour"
    d = RC.load("cleanup_10x9_beams")
    a = d["tiles"][..., 3]
    assert ((a > 0) & (a < 255)).any() and d["grid"].shape[1] == 3
    beams = np.isin(d["grid"][d["image_frames"]][:, 2], (7, 8, 9, 10)).reshape(len(d["image_frames"]), -1).any(axis=1)
    assert beams[1:].all()
    d = RC.load("treasurehunt_8x8_two_epochs")
    assert sorted(set(d["epoch"].tolist())) == [0, 1] and (d["win_vision"] * 2 + 1 > 8).any()
    assert d["tiles12"].shape[1:] == (12, 12, 4)


def test_atlas_from_png_paths_is_the_decoded_fixture():
    for name in RC.FIXTURES:
        d = RC.load(name)
        for i, sprite in enumerate(d["tile_names"]):
            assert np.array_equal(V.load_sprite(RC.sprite_path(str(sprite)), (16, 16)), d["tiles"][i]), sprite     # hero.png is mode P
            if "tiles12" in d:
                assert np.array_equal(V.load_sprite(RC.sprite_path(str(sprite)), (12, 12)), d["tiles12"][i]), sprite
        flags = V.tile_flags(d["tiles"])
        alpha = d["tiles"][..., 3].reshape(len(flags), -1)
        assert np.array_equal(flags & 1, (alpha.min(axis=1) == 255) * 1) and np.array_equal(flags >> 1, (alpha.max(axis=1) == 0) * 1)


# ------------------------------------------------------------------------------------------------------------- SpriteRenderer on a CPU world
def fixture_world(d, agent_factory, device="cpu", num_envs=1, tile_size=(16, 16)):
    """A ``Gridworld`` whose registered types are the fixture's (stand-in entities carrying the fixture's sprite files; the agents are the
    shipped example's class) inside a minimal stand-in for the Environment: what SpriteRenderer reads of it."""
    from sorrel_amd.entities.entity import Entity
    from sorrel_amd.worlds import Gridworld

    names = [str(n) for n in d["type_names"]]
    A = d["pos"].shape[1]
    agents = [agent_factory() for _ in range(A)]

    def cell(i, name):
        e = Entity()
        e.kind, e.value = name, float(i)
        e.sprite = RC.sprite_path(str(d["tile_names"][int(d["type_tile"][i])]))
        return e

    agent_ids = {i: n for i, n in enumerate(names) if n.split(":")[0] == type(agents[0]).__name__}
    default = cell(0, names[0])
    _, L, Hh, Ww = d["grid"].shape
    w = Gridworld(Hh, Ww, L, default, num_envs=num_envs, device=device)
    ids = np.zeros((len(names),), np.uint8)
    for i, name in enumerate(names):
        if i in agent_ids:
            proto = agents[0] if ":" not in name else agents[0].as_kind(name.split(":")[1])
            ids[i] = w.registry.register(proto)
        else:
            ids[i] = w.registry.register(cell(i, name))
    w.agent_layer = int(d["agent_layer"])
    w.agent_pos = torch.zeros((num_envs, A, 2), dtype=torch.uint8, device=device)
    for slot, a in enumerate(agents):
        a.slot, a._world = slot, w
    eng = types.SimpleNamespace(actions=torch.zeros((num_envs, A), dtype=torch.uint8, device=device),
                                state_at_pov=torch.zeros((num_envs, A), dtype=torch.uint8, device=device) if len(agent_ids) > 1 else None)
    env = types.SimpleNamespace(world=w, agents=agents, turn=0, epoch=1, _engine=eng)
    w._environment = env
    return env, ids


def agent_factories(d):
    from sorrel_amd.action.action_spec import ActionSpec

    moves = ["up", "down", "left", "right"]
    name = str(d["type_names"][-1]).split(":")[0]
    def sp(*sprites):       # (the fixtures carry the sprites their frames show, under the name of the file they resolve to; a direction no
        for sprite in sprites:          # agent ever took has no file here)
            if os.path.isfile(RC.sprite_path(sprite)):
                return RC.sprite_path(sprite)
        return None

    if name == "TreasurehuntAgent":
        from sorrel_amd.examples.treasurehunt.agents import TreasurehuntAgent

        def make():
            a = TreasurehuntAgent(None, ActionSpec(moves), None)
            a.sprite = sp("treasurehunt-hero.png")
            a.sprite_directions = [sp("agents-hero-back.png"), sp("agents-hero.png"), sp("agents-hero-left.png"), sp("agents-hero-right.png")]
            return a
    elif name == "TagAgent":
        from sorrel_amd.examples.tag.agents import TagAgent

        def make():
            a = TagAgent(None, ActionSpec(moves), None)
            a.sprite = sp("agents-hero.png")
            a._not_it_sprite_dirs = [sp("tag-hero-back.png", "agents-hero-back.png"), sp("tag-hero.png"), sp("tag-hero-left.png"), sp("tag-hero-right.png", "agents-hero-right.png")]
            a._it_sprite_dirs = [sp("tag-hero-back-g.png"), sp("tag-hero-g.png"), sp("tag-hero-left-g.png"), sp("tag-hero-right-g.png")]
            return a
    else:
        from sorrel_amd.examples.cleanup.agents import CleanupAgent

        def make():
            a = CleanupAgent(None, ActionSpec(moves + ["clean", "zap"]), None)
            a.sprite = sp("agents-hero.png")
            a.sprite_directions = [sp("agents-hero-back.png"), sp("agents-hero.png"), sp("agents-hero-left.png"), sp("agents-hero-right.png")]
            return a
    return make


def replay(d, env, ids, check):
    """Walk the fixture's frames in order, as an animated epoch does: put frame f's state into the world, ask for the pictures."""
    w, eng = env.world, env._engine
    dev = w.device
    shown = list(d["image_frames"])
    for f in range(d["grid"].shape[0]):
        w.grid.copy_(t(ids[d["grid"][f]]).to(dev)[None].expand_as(w.grid))
        w.agent_pos.copy_(t(d["pos"][f]).to(dev)[None].expand_as(w.agent_pos))
        if int(d["turn"][f]) == 0 and f > 0:
            env.epoch += 1
        env.turn = int(d["turn"][f])
        if env.turn > 0:
            eng.actions.copy_(t(d["actions"][f]).to(dev)[None].expand_as(eng.actions))
            if eng.state_at_pov is not None:
                eng.state_at_pov.copy_(t(ids[d["state_at_pov"][f]]).to(dev)[None].expand_as(eng.actions))
        check(f, shown.index(f) if f in shown else None)


def tile_names_shown(r, d):
    """The sprite every agent of env 0 shows, by file name (KEEP: the sprite of the type of its cell)."""
    w = r.world
    tiles = r.agent_tiles()[0].cpu().numpy()
    pos = w.agent_pos[0].cpu().numpy()
    cell_tile = r.atlas.type_tile[w.grid[0, w.agent_layer].cpu().numpy()[pos[:, 0], pos[:, 1]]]
    return [os.path.basename(r.atlas.names[int(c if x == V.KEEP else x)]) for x, c in zip(tiles, cell_tile)]


@pytest.mark.parametrize("name", RC.FIXTURES)
def test_sprite_renderer_follows_the_agents_sprites_on_a_cpu_world(name):
    d = RC.load(name)
    env, ids = fixture_world(d, agent_factories(d))
    r = V.SpriteRenderer(env)

    def check(f, k):
        # (by pixels: the reference's Tag agents show agents/assets/hero-left.png until their first tag and tag/assets/hero-left.png after
        # it -- two files with the same picture)
        shown = [V.load_sprite(RC.sprite_path(n), (16, 16)) for n in tile_names_shown(r, d)]
        assert np.array_equal(np.stack(shown), d["tiles"][d["agent_tile"][f]]), f"{name}: frame {f}"
        if k is not None:
            assert np.array_equal(r.frames()[0].numpy(), d["frame"][k]), f"{name}: frame {f}"
            assert np.array_equal(r.layers([0])[0].numpy(), d["planes"][k]), f"{name}: planes of frame {f}"

    replay(d, env, ids, check)
    if "win_loc" in d:
        for i, (loc, v) in enumerate(zip(d["win_loc"], d["win_vision"])):
            planes = V.render_sprite(env.world, location=(int(loc[0]), int(loc[1]), 0), vision=int(v))
            assert isinstance(planes, list) and len(planes) == 2 and all(p.dtype == np.uint8 for p in planes)
            assert np.array_equal(np.stack(planes), d[f"win{i}_planes"])
            assert np.array_equal(np.array(V.image_from_array(planes)), d[f"win{i}_frame"])
        assert np.array_equal(np.stack(V.render_sprite(env.world, tile_size=[12, 12])), d["t12_planes"])


def test_windows_around_the_agents():
    d = RC.load("treasurehunt_8x8_two_epochs")
    env, ids = fixture_world(d, agent_factories(d), num_envs=3)
    r = V.SpriteRenderer(env)
    replay(d, env, ids, lambda f, k: None)
    at = int(d["win_at"])
    win = r.windows(1, env_ids=[2, 0])
    assert tuple(win.shape) == (2, 2, 48, 48, 4)
    full = np.pad(d["frame"][list(d["image_frames"]).index(at)], ((16, 16), (16, 16), (0, 0)))
    wall = d["tiles"][int(d["oob_tile"])]
    for a, (y, x) in enumerate(d["pos"][at].astype(int)):
        box = full[y * 16:y * 16 + 48, x * 16:x * 16 + 48]
        inside = np.zeros((48, 48), bool)
        inside[max(0, 16 - y * 16):48 - max(0, (y + 2 - 8) * 16), max(0, 16 - x * 16):48 - max(0, (x + 2 - 8) * 16)] = True
        want = np.where(inside[..., None], box, np.tile(wall, (3, 3, 1)))
        assert np.array_equal(win[0, a].numpy(), want) and np.array_equal(win[1, a].numpy(), want)


def test_render_sprite_has_the_reference_shapes_and_dtypes():
    from sorrel_amd.entities import EmptyEntity, Gem, Wall
    from sorrel_amd.worlds import Gridworld

    w = Gridworld(5, 7, 2, EmptyEntity(), num_envs=2, device="cpu")
    w.add((0, 0, 0), Wall())
    w.add((2, 3, 1), Gem(1))
    layers = V.render_sprite(w)
    assert isinstance(layers, list) and len(layers) == 2
    assert all(isinstance(p, np.ndarray) and p.shape == (5 * 16, 7 * 16, 4) and p.dtype == np.uint8 for p in layers)
    box = V.render_sprite(w, location=(0, 0, 0), vision=2, tile_size=[8, 8], env=1)
    assert len(box) == 2 and all(p.shape == (5 * 8, 5 * 8, 4) and p.dtype == np.uint8 for p in box)
    with pytest.raises(IndexError):
        V.render_sprite(w, env=2)


def test_colour_fallback_is_deterministic_and_needs_no_image():
    from sorrel_amd.entities import EmptyEntity, Gem, Wall
    from sorrel_amd.worlds import Gridworld

    def world():
        w = Gridworld(4, 4, 2, EmptyEntity(), num_envs=1, device="cpu")
        w.add((0, 0, 0), Wall())
        w.add((1, 1, 1), Gem(3))
        return w

    a, b = V.SpriteRenderer(world()).atlas, V.SpriteRenderer(world()).atlas
    assert np.array_equal(a.tiles, b.tiles) and np.array_equal(a.type_tile, b.type_tile) and a.names == b.names
    colours = V.kind_colours(["EmptyEntity", "Wall", "Gem"])
    w = world()
    r = V.SpriteRenderer(w)
    frame = r.layers()[0].numpy()
    assert (frame[0, 16:32, 16:32] == 0).all(), "the default entity's kind is fully transparent"
    assert (frame[0, :16, :16] == [*colours["Wall"], 255]).all() and (frame[1, 16:32, 16:32] == [*colours["Gem"], 255]).all()
    assert np.array_equal(r.atlas.flags, V.tile_flags(r.atlas.tiles)) and set(r.atlas.flags.tolist()) == {1, 2}
    assert r.atlas.oob_tile == r.atlas.type_tile[w.registry.ids[Wall().type_key()]]
    w.add((2, 2, 1), Gem(7))          # a new type: the atlas follows registry.version
    assert r.atlas.version == w.registry.version and np.array_equal(r.frames()[0, 32:48, 32:48].numpy(), r.frames()[0, 16:32, 16:32].numpy())


def test_image_renderer_writes_the_frames_it_was_given(tmp_path):
    from PIL import Image, ImageSequence

    from sorrel_amd.entities import EmptyEntity, Gem, Wall
    from sorrel_amd.worlds import Gridworld

    w = Gridworld(4, 5, 2, Wall(), num_envs=2, device="cpu")
    ir = V.ImageRenderer("Demo", record_period=1, num_turns=3)
    added = []
    for turn in range(3):
        w.add((1 + turn % 2, 1 + turn, 1), Gem(1 + turn))
        w.add((turn, 0, 0), EmptyEntity())
        ir.add_image(w)
        added.append(V.renderer_of(w).frames([0])[0].numpy())
    assert len(ir.frames) == 3
    ir.save_gif(4, tmp_path / "gifs")
    assert ir.frames == []
    with Image.open(tmp_path / "gifs" / "Demo_epoch4.gif") as im:
        assert im.info["duration"] == 100 and im.info["loop"] == 0 and im.n_frames == 3
        got = [np.array(f.convert("RGBA")) for f in ImageSequence.Iterator(im)]
        im.seek(1)
        assert im.disposal_method == 2
    for g, a in zip(got, added):
        assert np.array_equal(g, a)
    sheet = V.SpriteRenderer.contact_sheet(torch.stack([V.renderer_of(w).frames()]))
    assert tuple(sheet.shape) == (1, 64, 160, 4) and np.array_equal(sheet[0, :, 80:].numpy(), V.renderer_of(w).frames([1])[0].numpy())


def test_unknown_actions_keep_the_sprite():
    """An action index beyond the sprite list keeps the current tile (the reference raises IndexError there)."""
    d = RC.load("cleanup_10x9_beams")
    env, ids = fixture_world(d, agent_factories(d))
    r = V.SpriteRenderer(env)
    env.turn = 1
    env._engine.actions.fill_(2)
    assert tile_names_shown(r, d) == ["agents-hero-left.png"] * 2
    for action in (4, 5, 9, 255):
        env.turn += 1
        env._engine.actions.fill_(action)
        assert tile_names_shown(r, d) == ["agents-hero-left.png"] * 2
    env.epoch, env.turn = env.epoch + 1, 0           # reset(): the agents outlive the epoch
    assert tile_names_shown(r, d) == ["agents-hero-left.png"] * 2


# ------------------------------------------------------------------------------------------------------------- module names, ABI
def test_compat_import_of_the_visualization_module_resolves():
    import sorrel_amd.compat as compat

    assert "utils.visualization" in compat.MIRRORED and "utils.visualization" not in compat.OUT_OF_SCOPE
    script = ("from sorrel.utils.visualization import ImageRenderer, render_sprite, image_from_array, animate_gif, plot, image_from_figure\n"
              "import sorrel_amd.utils.visualization as V\nassert ImageRenderer is V.ImageRenderer and render_sprite is V.render_sprite\nprint('ok')\n")
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "script.py"), "w") as fh:
            fh.write(script)
        out = subprocess.run([sys.executable, "-m", "sorrel_amd.compat", os.path.join(tmp, "script.py")], cwd=H.ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_header_declares_the_render_call_and_the_version_stands(built):
    import ctypes as C
    import re

    text = open(os.path.join(H.ROOT, "include", "sgw.h")).read()
    assert re.search(r"int sgw_render\(const sgw_render_desc\* desc, void\* stream\);", text) and "sgw_render" in N.EXPORTS
    macros = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+(SGW_[A-Z_0-9]+)\s+(0x[0-9A-Fa-f]+|\d+)\b", text)}
    assert (N.RENDER_COMPOSITE, N.RENDER_LAYERS, N.TILE_OPAQUE, N.TILE_CLEAR, N.TILE_KEEP) == tuple(
        macros[k] for k in ("SGW_RENDER_COMPOSITE", "SGW_RENDER_LAYERS", "SGW_TILE_OPAQUE", "SGW_TILE_CLEAR", "SGW_TILE_KEEP"))
    body = re.search(r"typedef struct sgw_render_desc \{(.*?)\} sgw_render_desc;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.split("*")[-1].split()[-1] for decl in body.split(";") if decl.strip() for f in decl.split(",")]
    assert fields == [name for name, _ in N.SgwRenderDesc._fields_]
    assert C.sizeof(N.SgwRenderDesc) == 9 * 8 + 3 * 8 + 12 * 4
    lib = N.load()
    assert lib.sgw_version() == b"sgw 0.3 (gfx950)"
    assert lib.sgw_render(None, None) == N.EINVAL and b"desc is NULL" in lib.sgw_last_error()
    d = N.SgwRenderDesc()
    assert lib.sgw_render(C.byref(d), None) == N.EINVAL and b"must not be NULL" in lib.sgw_last_error()
    d.grid = d.atlas = d.type_tile = d.out = 4096
    d.num_envs, d.layers, d.height, d.width, d.th, d.tw, d.n_tiles = 1, 9, 4, 4, 16, 16, 3
    assert lib.sgw_render(C.byref(d), None) == N.EINVAL and b"layers" in lib.sgw_last_error()
    d.layers, d.oob_tile = 2, 3
    assert lib.sgw_render(C.byref(d), None) == N.EINVAL and b"oob_tile" in lib.sgw_last_error()
    d.oob_tile, d.tw = 0, 65
    assert lib.sgw_render(C.byref(d), None) == N.EINVAL and b"tile" in lib.sgw_last_error()
    d.tw, d.width = 16, 2048
    assert lib.sgw_render(C.byref(d), None) == N.EINVAL and b"columns" in lib.sgw_last_error()


# ------------------------------------------------------------------------------------------------------------- the running reference
def _reference_child():
    """Random two- and three-layer worlds of the reference's own Treasurehunt / Cleanup entities, rendered by the reference's
    ``render_sprite`` + ``image_from_array`` and by the torch path from the same cell ids."""
    ref_loader.install()
    import sorrel.examples.cleanup.entities as ce
    import sorrel.examples.treasurehunt.entities as te
    import sorrel.utils.visualization as ref_vis
    from sorrel.examples.cleanup.agents import CleanBeam, ZapBeam
    from sorrel.worlds import Gridworld

    rng = np.random.default_rng(7)
    makers = [te.EmptyEntity, te.Wall, te.Sand, lambda: te.Gem(1), lambda: te.Food(1), lambda: te.Bone(1), ce.River, ce.Pollution,
              ce.AppleTree, ce.Apple, CleanBeam, ZapBeam, ce.Wall]
    protos = [m() for m in makers]
    for case, (Hh, Ww, L, ts) in enumerate([(5, 6, 2, 16), (4, 9, 3, 16), (7, 3, 3, 12), (3, 3, 1, 16)]):
        world = Gridworld(Hh, Ww, L, te.EmptyEntity())
        ids = rng.integers(0, len(makers), size=(L, Hh, Ww))
        ids[:, 0, 0] = 1                          # (the reference looks the Wall up for tiles outside the map)
        for (z, y, x), i in np.ndenumerate(ids):
            world.add((y, x, z), makers[i]())
        atlas = np.stack([V.load_sprite(p.sprite, (ts, ts)) for p in protos])
        tt = torch.zeros(256, dtype=torch.int64)
        tt[:len(protos)] = torch.arange(len(protos))
        grid = torch.from_numpy(ids.astype(np.uint8))[None]
        planes = ref_vis.render_sprite(world, tile_size=[ts, ts])
        assert np.array_equal(V.render_torch(grid, t(atlas), tt, 1, per_layer=True)[0].numpy(), np.stack(planes)), case
        assert np.array_equal(V.render_torch(grid, t(atlas), tt, 1)[0].numpy(), np.array(ref_vis.image_from_array(planes))), case
        loc, v = (int(rng.integers(0, Hh)), int(rng.integers(0, Ww))), int(rng.integers(1, 5))
        planes = ref_vis.render_sprite(world, location=(loc[0], loc[1], 0), vision=v, tile_size=[ts, ts])
        c = torch.tensor([[loc]], dtype=torch.int16)
        assert np.array_equal(V.render_torch(grid, t(atlas), tt, 1, centres=c, vision=v, per_layer=True)[0, 0].numpy(), np.stack(planes)), case
        assert np.array_equal(V.render_torch(grid, t(atlas), tt, 1, centres=c, vision=v)[0, 0].numpy(), np.array(ref_vis.image_from_array(planes))), case
    print("reference ok")


@pytest.mark.skipif(not ref_loader.reference_available(), reason="the reference checkout is not on this machine")
def test_torch_path_matches_the_running_reference():
    """(In a process of its own: the reference is imported as ``sorrel``, the name ``sorrel_amd.compat`` aliases.)"""
    out = subprocess.run([sys.executable, "-B", os.path.abspath(__file__)], cwd=H.ROOT, capture_output=True, text=True,
                         env=dict(os.environ, PYTHONPATH=H.ROOT))
    assert out.returncode == 0 and "reference ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


if __name__ == "__main__":
    _reference_child()
