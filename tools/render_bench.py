#!/usr/bin/env python3
"""Sprite frames on the device: the sgw_render kernel against the product's torch path and against ``Tensor.fill_`` of the output's size
(the write ceiling README uses).  Prints the text of profiles/render_frames.txt.

usage: python tools/render_bench.py [--reps 20]

Workloads: composited frames of the 32 x 32 x 2 Treasurehunt world at 16 x 16 tiles for 1 024 and 4 096 envs, and the vision-3 windows of
8 agents for 4 096 envs.  Each is timed with device events after warm-up, kernel and fill_ alternating in one loop; the torch path
(seconds per call) gets one warm-up and three timed calls.  Before any timing the kernel's frames are compared with the torch path's."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sorrel_amd.examples.treasurehunt.entities import EmptyEntity  # noqa: E402
from sorrel_amd.examples.treasurehunt.env import TreasurehuntEnv  # noqa: E402
from sorrel_amd.examples.treasurehunt.main import make_config  # noqa: E402
from sorrel_amd.examples.treasurehunt.world import TreasurehuntWorld  # noqa: E402
from sorrel_amd.utils import visualization as V  # noqa: E402

SPRITES = os.path.join(ROOT, "tests", "golden", "render", "sprites")


def timed(fn, reps, other=None):
    """Median / min ms of ``fn`` over ``reps`` calls (device events); ``other`` runs between them and is timed the same way."""
    a, b = [], []
    for _ in range(reps):
        for f, out in ((fn, a), (other, b)):
            if f is None:
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--envs", type=int, nargs="*", default=[1024, 4096])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("render_bench needs the GPU: a timing taken anywhere else says nothing")
    print(f"device: {torch.cuda.get_device_name(0)}; ms per call, median (min) of {args.reps} calls after warm-up; device events")
    rows = []
    for E in args.envs:
        cfg = make_config(32, 32, 8, 3, spawn_prob=0.05, max_turns=20)
        env = TreasurehuntEnv(TreasurehuntWorld(cfg, EmptyEntity(), num_envs=E, device="cuda:0", seed=1), cfg)
        for _ in range(10):
            env.take_turn()
        dressed = os.path.isdir(SPRITES)
        if dressed:                 # the reference's Treasurehunt sprites (test fixtures); without them: the flat colour tiles
            files = dict(Wall="wall", Sand="sand", Gem="gem", Food="food", Bone="bone", EmptyEntity="empty", TreasurehuntAgent="hero")
            for p in env.world.registry.prototypes:
                if type(p).__name__ in files:
                    p.sprite = os.path.join(SPRITES, f"treasurehunt-{files[type(p).__name__]}.png")
        r = V.SpriteRenderer(env)
        a, w = r.atlas, env.world
        if E == args.envs[0]:
            print(f"tiles: {'the reference sprites of tests/golden/render/sprites' if dressed else 'flat colour tiles'}: {a.tiles.shape[0]} tiles, flags {a.flags.tolist()}")
        tiles = r.agent_tiles()

        def torch_path(centres=None, vision=0):
            return V.render_torch(w.grid, r._dev["atlas"], r._dev["type_tile"], a.oob_tile, w.agent_pos, w.agent_layer, tiles, None, centres, vision)

        work = [("frames", lambda out=None: r.frames(out=out), lambda: torch_path())]
        if E == max(args.envs):
            centres = w.agent_pos.to(torch.int16)
            work.append(("windows(vision=3) x 8 agents", lambda out=None: r._render(None, centres=centres, vision=3, out=out), lambda: torch_path(centres, 3)))
        for label, kernel, reference in work:
            out = kernel()
            torch.cuda.synchronize()
            want = reference()
            assert torch.equal(out, want), f"{label}: the kernel's frames differ from the torch path's"
            del want
            for _ in range(3):
                kernel(out)
                out.fill_(7)
            kernel(out)
            k_ms, f_ms = timed(lambda: kernel(out), args.reps, lambda: out.fill_(7))
            t_ms, _ = timed(reference, 3)
            gib = out.numel() / 2 ** 30
            km, fm, tm = statistics.median(k_ms), statistics.median(f_ms), statistics.median(t_ms)
            rows.append((E, label, gib, km, min(k_ms), fm, min(f_ms), tm))
            print(f"E={E:5d} {label:30s} out {gib:6.3f} GiB | kernel {km:8.3f} ({min(k_ms):8.3f}) = {gib * 2 ** 30 / km / 1e6:7.1f} GB/s | "
                  f"fill_ {fm:8.3f} ({min(f_ms):8.3f}) = {gib * 2 ** 30 / fm / 1e6:7.1f} GB/s | kernel at {fm / km:5.2f} of fill_ | "
                  f"torch path {tm:10.2f} = {tm / km:7.1f} x the kernel", flush=True)
            del out
            torch.cuda.empty_cache()
    assert all(r[3] < r[7] for r in rows), "the kernel must be faster than the torch path on every workload"
    print("the kernel is faster than the torch path on every workload")


if __name__ == "__main__":
    main()
