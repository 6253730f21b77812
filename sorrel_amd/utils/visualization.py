"""Sprite frames of the batched world: ``sorrel/utils/visualization.py`` (``render_sprite``, ``image_from_array``, ``ImageRenderer``,
``animate_gif``, ``plot``, ``image_from_figure``) plus the batched form, ``SpriteRenderer``.

A frame is a gather (tile of every cell), a paste of the layers bottom-up and a streaming store.  On a GPU world that is one
``sgw_render`` launch over ``grid[E, L, H, W]`` (``sorrel_amd/csrc/render.h``); on a CPU world the same integers are computed with
torch (``render_torch``), which is also what the kernel is tested and timed against.  The paste is PIL's
``Image.paste(layer, (0, 0), mask=layer)`` on RGBA images, for each of the four bytes (``a`` = the pasted pixel's alpha)::

    t = dst * (255 - a) + src * a + 128;   out = ((t >> 8) + t) >> 8

Tiles.  A type whose prototype carries a ``sprite`` path is loaded the way the reference loads it,
``Image.open(path).resize(tile_size).convert("RGBA")`` (needs Pillow).  A type without one gets a flat opaque tile in the colour
``RGBObservationSpec.generate_map`` gives its kind among the kinds registered so far; a sprite-less type of the default entity's kind
is fully transparent.  The shipped examples carry no image files and render with these colours.  Tiles outside the map show the
first ``Wall`` kind's tile, as in the reference.

Agents.  What an agent shows is what the reference's ``agent.sprite`` would hold: the constructor's sprite until its first
``movement(action)``, then ``sprite_directions[action]`` -- for the actions the class lists in ``sprite_switch_actions`` (None: every
action; Treasurehunt: none, its ``act`` never calls ``movement``; Cleanup: the four moves).  A class whose sprite list depends on
its state (Tag) gives one list per state kind (``Agent.sprite_table``); the state looked up is the one the agent had when it acted
(the engine's ``state_at_pov``), so a tagged agent keeps its old colour until it moves.  The tiles ``[E, A]`` are kept by the renderer
and brought up to date from the engine's ``actions`` when a frame is asked for -- nothing runs per turn when nobody renders.  They are
exact when a frame is taken every turn (``run_experiment(animate=True)``) or every action switches the sprite; otherwise only the last
turn's action is seen.  They persist across ``reset()``.  An action index without an entry in the list keeps the current tile (the
reference raises ``IndexError`` there).
"""
from __future__ import annotations

import os
from pathlib import Path
from typing import Optional, Sequence

import numpy as np
import torch

KEEP = 0xFFFF
_FRAMES_PER_CHUNK = 64      # render_torch: frames pasted at a time (bounds the int32 temporaries)


def _need_pillow(what: str):
    try:
        from PIL import Image
    except ImportError as exc:      # pragma: no cover - Pillow is present wherever the tests run
        raise ImportError(f"{what} needs Pillow (PIL); device rendering and the flat colour tiles work without it") from exc
    return Image


# --------------------------------------------------------------------------------------------------------------- the integers
def paste(dst: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
    """PIL's masked paste of RGBA ``src`` over ``dst`` (uint8 ``[..., 4]``), all four bytes, in integers."""
    d, s = dst.to(torch.int32), src.to(torch.int32)
    a = s[..., 3:4]
    t = d * (255 - a) + s * a + 128
    return (((t >> 8) + t) >> 8).to(torch.uint8)


def composite(planes: torch.Tensor) -> torch.Tensor:
    """``[m, L, h, w, 4]`` -> ``[m, h, w, 4]``: layer 0 as it is, the others pasted over it bottom-up."""
    acc = planes[:, 0]
    for l in range(1, planes.shape[1]):
        acc = paste(acc, planes[:, l])
    return acc


def render_torch(grid, atlas, type_tile, oob_tile, agent_pos=None, agent_layer=0, agent_tile=None, env_ids=None, centres=None,
                 vision=0, per_layer=False, out=None):
    """The frames ``sgw_render`` produces, with torch ops on whatever device the tensors live on.

    ``grid`` uint8 ``[E, L, H, W]``, ``atlas`` uint8 ``[n_tiles, th, tw, 4]``, ``type_tile`` integer ``[256]``, ``agent_pos`` uint8
    ``[E, A, 2]`` with ``agent_tile`` integer ``[E, A]`` (``KEEP`` or any value >= n_tiles: the cell's own tile), ``env_ids`` int64 ``[n]``
    (None: all), ``centres`` integer ``[n, k, 2]`` with ``vision`` (None: whole maps).  Returns uint8 ``[n]([k])([L])[rows*th][cols*tw][4]``."""
    E, L, H, W = grid.shape
    nt, th, tw = atlas.shape[:3]
    dev = grid.device
    sel = torch.arange(E, device=dev) if env_ids is None else env_ids.to(dev).long()
    n = int(sel.shape[0])
    k = 1 if centres is None else int(centres.shape[1])
    rows, cols = (H, W) if centres is None else (2 * vision + 1, 2 * vision + 1)
    planes = L if per_layer else 1
    shape = (n,) + ((k,) if centres is not None else ()) + ((L,) if per_layer else ()) + (rows * th, cols * tw, 4)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    flat = out.view(n * k, planes, rows * th, cols * tw, 4)
    tt = type_tile.to(dev).long()
    step = max(1, _FRAMES_PER_CHUNK // k)
    for lo in range(0, n, step):
        s = sel[lo:lo + step]
        m = int(s.shape[0])
        tiles = tt[grid[s].long()]                                              # [m, L, H, W]
        tiles = torch.where(tiles >= nt, torch.full_like(tiles, oob_tile), tiles)
        if agent_pos is not None and agent_tile is not None:
            at = agent_tile[s].long() & 0xFFFF                                  # [m, A]
            pos = agent_pos[s].long()
            ok = (at < nt) & (pos[..., 0] < H) & (pos[..., 1] < W)
            mi = torch.arange(m, device=dev)[:, None].expand_as(at)
            tiles[mi[ok], agent_layer, pos[..., 0][ok], pos[..., 1][ok]] = at[ok]
        if centres is not None:
            c = centres[lo:lo + step].to(dev).long()                           # [m, k, 2]
            d = torch.arange(-vision, vision + 1, device=dev)
            ys, xs = c[..., 0, None] + d, c[..., 1, None] + d                   # [m, k, R]
            inside = ((ys >= 0) & (ys < H))[..., :, None] & ((xs >= 0) & (xs < W))[..., None, :]      # [m, k, R, C]
            mi = torch.arange(m, device=dev)[:, None, None, None]
            t = tiles[mi, :, ys.clamp(0, H - 1)[..., :, None], xs.clamp(0, W - 1)[..., None, :]]     # [m, k, R, C, L]
            t = torch.where(inside[..., None], t, torch.full_like(t, oob_tile))
            tiles = t.permute(0, 1, 4, 2, 3).reshape(m * k, L, rows, cols)
        px = atlas.to(dev)[tiles]                                               # [f, L, rows, cols, th, tw, 4]
        px = px.permute(0, 1, 2, 4, 3, 5, 6).reshape(tiles.shape[0], L, rows * th, cols * tw, 4)
        flat[lo * k:lo * k + tiles.shape[0]] = px if per_layer else composite(px)[:, None]
    return out


# --------------------------------------------------------------------------------------------------------------- the atlas
def load_sprite(path, tile_size) -> np.ndarray:
    """uint8 ``(th, tw, 4)`` of a sprite file, loaded as the reference loads it."""
    Image = _need_pillow(f"loading the sprite {path}")
    th, tw = int(tile_size[0]), int(tile_size[1])
    with Image.open(os.path.expanduser(str(path))) as im:
        return np.array(im.resize((tw, th)).convert("RGBA"), dtype=np.uint8)


def kind_colours(kinds: Sequence[str]) -> dict:
    """kind -> uint8 RGB, the colours ``RGBObservationSpec.generate_map`` gives the list."""
    from sorrel_amd.observation.observation_spec import RGBObservationSpec

    return {k: np.asarray(v, dtype=np.uint8) for k, v in RGBObservationSpec.generate_map(None, list(kinds)).items()}


def tile_flags(tiles: np.ndarray) -> np.ndarray:
    """uint8 ``[n_tiles]``: 1 = every alpha is 255, 2 = every alpha is 0 (``SGW_TILE_OPAQUE`` / ``SGW_TILE_CLEAR``)."""
    a = tiles[..., 3].reshape(tiles.shape[0], -1)
    return ((a == 255).all(axis=1) * 1 + (a == 0).all(axis=1) * 2).astype(np.uint8)


class Atlas:
    """The tiles of a world's registered types (and of its agents' sprite lists) at one ``registry.version``."""

    def __init__(self, world, agents, tile_size):
        th, tw = int(tile_size[0]), int(tile_size[1])
        if not (1 <= th <= 64 and 1 <= tw <= 64):
            raise ValueError(f"tile_size {tuple(tile_size)} outside 1..64")
        protos = world.registry.prototypes
        kinds = list(dict.fromkeys(p.kind for p in protos))
        colours = kind_colours(kinds)
        default_kind = world.default_entity.kind
        self.names, self._tiles, self._index = [], [], {}

        def tile_of(sprite, kind):
            if sprite is not None and not isinstance(sprite, np.ndarray) and str(sprite) in ("", "."):
                sprite = None
            if sprite is None:
                key = ("clear",) if kind == default_kind else ("flat", kind)
            elif isinstance(sprite, np.ndarray):
                key = ("array", sprite.tobytes(), sprite.shape)
            else:
                key = ("file", str(sprite))
            if key not in self._index:
                if key[0] == "clear":
                    px = np.zeros((th, tw, 4), np.uint8)
                elif key[0] == "flat":
                    px = np.empty((th, tw, 4), np.uint8)
                    px[..., :3], px[..., 3] = colours.get(kind, np.zeros(3, np.uint8)), 255
                elif key[0] == "array":
                    px = np.ascontiguousarray(sprite, dtype=np.uint8)
                    if px.shape != (th, tw, 4):
                        raise ValueError(f"a sprite array must be uint8 {(th, tw, 4)}, not {px.shape}")
                else:
                    px = load_sprite(sprite, (th, tw))
                self._index[key] = len(self._tiles)
                self._tiles.append(px)
                self.names.append(key[1] if key[0] in ("file", "flat") else key[0])
            return self._index[key]

        type_tile = [tile_of(getattr(p, "sprite", None), p.kind) for p in protos]
        walls = [t for t, p in zip(type_tile, protos) if p.kind == "Wall"]
        self.oob_tile = walls[0] if walls else type_tile[world.default_type]
        # per agent slot: [type id][action] -> tile (KEEP: the action does not switch the sprite, or the list has no entry for it)
        n_act = max([a.action_spec.n_actions for a in agents], default=0)
        self.agent_table = np.full((len(agents), len(protos), n_act + 1), KEEP, np.int32)
        self.agent_type = np.zeros((len(agents),), np.int64)
        for slot, agent in enumerate(agents):
            self.agent_type[slot] = world.registry.ids.get(agent.type_key(), 0)
            switch = agent.sprite_switch_actions
            table = agent.sprite_table()
            for t, p in enumerate(protos):
                if type(p) is not type(agent) or p.kind not in table:
                    continue
                sprites = table[p.kind]
                for action in range(agent.action_spec.n_actions):
                    if (switch is None or action in switch) and action < len(sprites):
                        self.agent_table[slot, t, action] = tile_of(sprites[action], p.kind)
        self.tiles = np.stack(self._tiles)
        self.flags = tile_flags(self.tiles)
        self.type_tile = np.full((256,), self.oob_tile, np.int64)
        self.type_tile[:len(protos)] = type_tile
        self.version = world.registry.version


# --------------------------------------------------------------------------------------------------------------- the renderer
class SpriteRenderer:
    """Frames of many envs at once.  ``world_or_env``: a ``Gridworld`` or the ``Environment`` around it (with the environment the
    agents show their own sprites, see the module text)."""

    def __init__(self, world_or_env, tile_size=(16, 16)):
        if hasattr(world_or_env, "world") and hasattr(world_or_env, "agents"):
            self.env, self.world = world_or_env, world_or_env.world
        else:
            self.world, self.env = world_or_env, getattr(world_or_env, "_environment", None)
        self.tile_size = (int(tile_size[0]), int(tile_size[1]))
        self._atlas = None
        self._dev = {}
        self._tiles = None           # int32 [E, A]: what every agent shows
        played = self.env is not None and (self.env.turn > 0 or self.env.epoch > 1)
        self._stamp = None if played else self._now()

    def _now(self):
        return None if self.env is None else (int(self.env.epoch), int(self.env.turn))

    # ---------------------------------------------------------------- tables
    @property
    def atlas(self) -> Atlas:
        w = self.world
        if self._atlas is None or self._atlas.version != w.registry.version:
            agents = list(self.env.agents) if self.env is not None else []
            a = Atlas(w, agents, self.tile_size)
            dev = w.device
            self._atlas = a
            self._dev = dict(
                atlas=torch.from_numpy(a.tiles).to(dev).contiguous(), flags=torch.from_numpy(a.flags).to(dev),
                type_tile=torch.from_numpy(a.type_tile).to(dev), type_tile16=torch.from_numpy(a.type_tile.astype(np.uint16).view(np.int16)).to(dev),
                agent_table=torch.from_numpy(a.agent_table).to(dev), agent_type=torch.from_numpy(a.agent_type).to(dev))
        return self._atlas

    def agent_tiles(self) -> Optional[torch.Tensor]:
        """int32 ``[E, A]``: the tile every agent shows now (``KEEP``: the tile of its cell's type), or None without agents."""
        w, env = self.world, self.env
        if env is None or w.agent_pos is None or w.agent_layer is None or not env.agents:
            return None
        self.atlas
        E, A = w.num_envs, len(env.agents)
        if self._tiles is None or tuple(self._tiles.shape) != (E, A):
            self._tiles = torch.full((E, A), KEEP, dtype=torch.int32, device=w.device)
        now = self._now()
        if now != self._stamp and env._engine is not None:
            eng = env._engine
            table = self._dev["agent_table"]                                    # [A, T, n_act + 1]
            act = eng.actions.long().clamp(max=table.shape[2] - 1)
            if eng.state_at_pov is not None:
                state = eng.state_at_pov.long().clamp(max=table.shape[1] - 1)
            else:
                state = self._dev["agent_type"][None, :].expand(E, A)
            new = table[torch.arange(A, device=w.device)[None, :], state, act]
            self._tiles = torch.where(new != KEEP, new, self._tiles)
        self._stamp = now
        return self._tiles

    # ---------------------------------------------------------------- rendering
    def _render(self, env_ids=None, centres=None, vision=0, per_layer=False, out=None) -> torch.Tensor:
        w = self.world
        a = self.atlas
        dev = w.device
        E, L, H, W = w.num_envs, w.layers, w.height, w.width
        th, tw = self.tile_size
        if env_ids is not None:
            env_ids = torch.as_tensor(env_ids, dtype=torch.int64, device=dev).reshape(-1).contiguous()
            if env_ids.numel() and (int(env_ids.min()) < 0 or int(env_ids.max()) >= E):
                raise IndexError(f"env_ids outside [0, {E})")
        n = E if env_ids is None else int(env_ids.shape[0])
        rows, cols = (H, W) if centres is None else (2 * vision + 1, 2 * vision + 1)
        k = 1 if centres is None else int(centres.shape[1])
        shape = (n,) + ((k,) if centres is not None else ()) + ((L,) if per_layer else ()) + (rows * th, cols * tw, 4)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=dev)
        elif tuple(out.shape) != shape or out.dtype != torch.uint8 or out.device != dev or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous uint8 tensor {shape} on {dev}")
        tiles = self.agent_tiles()
        if centres is not None:
            centres = centres.to(device=dev, dtype=torch.int16).contiguous()
        if dev.type != "cuda":
            return render_torch(w.grid, self._dev["atlas"], self._dev["type_tile"], a.oob_tile, w.agent_pos if tiles is not None else None,
                                w.agent_layer or 0, tiles, env_ids, centres, vision, per_layer, out)
        from sorrel_amd import _native as N

        tiles16 = None if tiles is None else tiles.to(torch.int16).contiguous()
        d = N.SgwRenderDesc()
        d.grid, d.atlas, d.tile_flags = w.grid.data_ptr(), self._dev["atlas"].data_ptr(), self._dev["flags"].data_ptr()
        d.type_tile = self._dev["type_tile16"].data_ptr()
        if tiles16 is not None:
            d.agent_pos, d.agent_tile = w.agent_pos.data_ptr(), tiles16.data_ptr()
            d.num_agents, d.agent_layer = int(tiles16.shape[1]), int(w.agent_layer)
        d.env_ids = None if env_ids is None else env_ids.data_ptr()
        d.centres = None if centres is None else centres.data_ptr()
        d.out = out.data_ptr()
        d.num_envs, d.n, d.grid_env_stride = E, n, int(w.grid.stride(0))
        d.layers, d.height, d.width = L, H, W
        d.n_tiles, d.th, d.tw = int(a.tiles.shape[0]), th, tw
        d.k, d.vision, d.oob_tile = k, int(vision), int(a.oob_tile)
        d.mode = N.RENDER_LAYERS if per_layer else N.RENDER_COMPOSITE
        N.launch("sgw_render", d, dev)
        return out

    def frames(self, env_ids=None, out=None) -> torch.Tensor:
        """uint8 ``[n, H * th, W * tw, 4]``: the composited frame of every selected env (None: all), on the world's device."""
        return self._render(env_ids, out=out)

    def layers(self, env_ids=None) -> torch.Tensor:
        """uint8 ``[n, L, H * th, W * tw, 4]``: one plane per layer (what ``render_sprite`` returns for one env)."""
        return self._render(env_ids, per_layer=True)

    def windows(self, vision: int, agents=None, env_ids=None, centres=None, per_layer=False) -> torch.Tensor:
        """uint8 ``[n, k, (2v+1) * th, (2v+1) * tw, 4]``: the composited box of ``2 * vision + 1`` tiles around every agent of ``agents``
        (slots; None: all) -- or around ``centres`` (integer ``[n, k, 2]`` (y, x)) -- in every selected env.  Tiles outside the map
        show the ``Wall`` tile."""
        w = self.world
        if not 0 <= int(vision) <= 511:
            raise ValueError("vision outside 0..511")
        if centres is None:
            pos = w.agent_pos if env_ids is None else w.agent_pos[torch.as_tensor(env_ids, dtype=torch.int64, device=w.device).reshape(-1)]
            if agents is not None:
                pos = pos[:, torch.as_tensor(list(agents), dtype=torch.int64, device=w.device)]
            centres = pos.to(torch.int16)
        else:
            centres = torch.as_tensor(centres, device=w.device).to(torch.int16)
        n = w.num_envs if env_ids is None else int(torch.as_tensor(env_ids).numel())
        if centres.dim() != 3 or centres.shape[0] != n or centres.shape[2] != 2:
            raise ValueError(f"centres must be [{n}, k, 2]")
        return self._render(env_ids, centres=centres, vision=int(vision), per_layer=per_layer)

    # ---------------------------------------------------------------- files
    @staticmethod
    def contact_sheet(frames: torch.Tensor) -> torch.Tensor:
        """``[T, n, h, w, 4]`` -> ``[T, r * h, c * w, 4]``: the n envs of every turn side by side (c = ceil(sqrt(n)); empty slots stay
        transparent black)."""
        T, n, h, w, _ = frames.shape
        c = int(np.ceil(np.sqrt(n)))
        r = (n + c - 1) // c
        sheet = torch.zeros((T, r * c, h, w, 4), dtype=frames.dtype, device=frames.device)
        sheet[:, :n] = frames
        return sheet.view(T, r, c, h, w, 4).permute(0, 1, 3, 2, 4, 5).reshape(T, r * h, c * w, 4)

    @staticmethod
    def to_gif(path, frames) -> None:
        """Write uint8 RGBA frames ``[T, h, w, 4]`` (tensor or array) as a GIF with the reference's parameters (100 ms per frame,
        disposal 2, endless loop)."""
        Image = _need_pillow("writing a GIF")
        arr = frames.cpu().numpy() if torch.is_tensor(frames) else np.asarray(frames)
        if arr.ndim != 4 or arr.shape[3] != 4 or arr.shape[0] < 1:
            raise ValueError("to_gif wants frames [T, h, w, 4]")
        images = [Image.fromarray(np.ascontiguousarray(f), mode="RGBA") for f in arr]
        _save_gif(images, path)


def _save_gif(images, path) -> None:
    path = os.path.expanduser(str(path))
    Path(os.path.dirname(path) or ".").mkdir(parents=True, exist_ok=True)
    images[0].save(path, format="GIF", append_images=images[1:], save_all=True, duration=100, disposal=2, loop=0)


def renderer_of(world, tile_size=(16, 16)) -> SpriteRenderer:
    """The world's own renderer for a tile size (one per size: it carries what the agents show)."""
    key = (int(tile_size[0]), int(tile_size[1]))
    cache = world.__dict__.setdefault("_sprite_renderers", {})
    if key not in cache:
        cache[key] = SpriteRenderer(getattr(world, "_environment", None) or world, key)
    return cache[key]


# --------------------------------------------------------------------------------------------------------------- reference names
def render_sprite(world, location: Optional[Sequence] = None, vision: Optional[int] = None, tile_size=[16, 16], env: int = 0):
    """The layers of one env as a list of ``L`` uint8 arrays ``(h, w, 4)``: the whole map, or -- with ``location`` and ``vision`` --
    the ``2 * vision + 1`` tiles around ``location`` (``visualization.py:27-141``).  ``env`` picks the env of the batch."""
    r = renderer_of(world, tile_size)
    if vision is None or location is None:
        planes = r.layers([env])[0]
    else:
        loc = tuple(location.to_tuple()) if hasattr(location, "to_tuple") else tuple(location)
        centres = torch.tensor([[[int(loc[0]), int(loc[1])]]], dtype=torch.int16)
        planes = r.windows(int(vision), env_ids=[env], centres=centres, per_layer=True)[0, 0]
    planes = planes.cpu().numpy()
    return [planes[z] for z in range(planes.shape[0])]


def plot(image) -> None:
    """Show an image or a list of layers with Matplotlib (``visualization.py:144-157``)."""
    from matplotlib import pyplot as plt

    for layer in ([image] if isinstance(image, np.ndarray) else image):
        plt.imshow(layer)
    plt.show()


def image_from_array(image):
    """PIL image of one RGBA array, or of a list of layers pasted bottom-up (``visualization.py:160-176``)."""
    Image = _need_pillow("image_from_array")
    if isinstance(image, np.ndarray):
        return Image.fromarray(image, mode="RGBA")
    output = Image.fromarray(image[0], mode="RGBA")
    for layer in image[1:]:
        nxt = Image.fromarray(layer, mode="RGBA")
        output.paste(nxt, (0, 0), mask=nxt)
    return output


def image_from_figure(fig):
    """A Matplotlib figure as a PIL image (``visualization.py:179-196``)."""
    import io

    Image = _need_pillow("image_from_figure")
    buf = io.BytesIO()
    fig.savefig(buf)
    buf.seek(0)
    return Image.open(buf)


def animate_gif(frames, filename: str, folder) -> None:
    """PIL frames -> ``<folder>/<filename>.gif`` (``visualization.py:199-224``)."""
    _need_pillow("animate_gif")
    _save_gif(list(frames), os.path.join(str(folder), filename + ".gif"))


class ImageRenderer:
    """The reference's frame container (``visualization.py:227-273``).  ``frames`` holds uint8 RGBA tensors on the world's device
    (one composited frame per ``add_image``); they become PIL images when the GIF is written."""

    def __init__(self, experiment_name: str, record_period: int, num_turns: int):
        self.experiment_name = experiment_name
        self.record_period = record_period
        self.num_turns = num_turns
        self.frames = []

    def clear(self) -> None:
        del self.frames[:]

    def add_image(self, world, env: int = 0) -> None:
        self.frames.append(renderer_of(world).frames([env])[0])

    def save_gif(self, epoch: int, folder) -> None:
        SpriteRenderer.to_gif(os.path.join(str(folder), f"{self.experiment_name}_epoch{epoch}.gif"), torch.stack(self.frames))
        self.clear()
