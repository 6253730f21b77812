"""What the render tests share: the fixtures of ``tests/golden/render`` (``tools/make_render_golden.py``) and the cases every
implementation is put through.  Not collected by pytest (no ``test_`` prefix)."""
import glob
import os

import numpy as np

from tests import helpers as H

RENDER_DIR = os.path.join(H.GOLDEN_DIR, "render")
SPRITE_DIR = os.path.join(RENDER_DIR, "sprites")
FIXTURES = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(RENDER_DIR, "*.npz")))


def load(name):
    with np.load(os.path.join(RENDER_DIR, name + ".npz")) as d:
        return {k: d[k] for k in d.files}


def type_tile256(d, tiles_key="tiles"):
    tt = np.full((256,), int(d["oob_tile"]), np.int64)
    tt[:len(d["type_tile"])] = d["type_tile"]
    return tt


def cases(d):
    """Every picture a fixture holds, as ``(label, render arguments, expected array)``: the arguments are those of
    ``visualization.render_torch`` after ``grid, atlas, type_tile, oob_tile`` (numpy; the caller moves them where it renders)."""
    out = []
    frames = d["image_frames"]
    common = dict(agent_pos=d["pos"][frames], agent_layer=int(d["agent_layer"]), agent_tile=d["agent_tile"][frames].astype(np.int32))
    out.append(("planes", "tiles", d["grid"][frames], dict(common, per_layer=True), d["planes"]))
    out.append(("frames", "tiles", d["grid"][frames], dict(common), d["frame"]))
    if "win_loc" in d:
        at = int(d["win_at"])
        one = dict(agent_pos=d["pos"][at:at + 1], agent_layer=int(d["agent_layer"]), agent_tile=d["agent_tile"][at:at + 1].astype(np.int32))
        for i, (loc, v) in enumerate(zip(d["win_loc"], d["win_vision"])):
            c = np.asarray(loc, np.int16).reshape(1, 1, 2)
            out.append((f"window {i} planes", "tiles", d["grid"][at:at + 1], dict(one, centres=c, vision=int(v), per_layer=True), d[f"win{i}_planes"][None, None]))
            out.append((f"window {i} frame", "tiles", d["grid"][at:at + 1], dict(one, centres=c, vision=int(v)), d[f"win{i}_frame"][None, None]))
        out.append(("12 x 12 planes", "tiles12", d["grid"][at:at + 1], dict(one, per_layer=True), d["t12_planes"][None]))
        out.append(("12 x 12 frame", "tiles12", d["grid"][at:at + 1], dict(one), d["t12_frame"][None]))
    return out


def sprite_path(name: str) -> str:
    return os.path.join(SPRITE_DIR, name)
