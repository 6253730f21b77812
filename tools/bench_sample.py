#!/usr/bin/env python3
"""Replay batches on the device: ``sgw_sample`` against the torch indexing path it replaces.  Prints the text of
profiles/replay_sample.txt.

usage: python tools/bench_sample.py [--reps 200] [--envs 65536] [--batches B ...] [--frames F ...] [--out FILE]

Ring: a ``Buffer`` of the config-3 window (``treasurehunt_spec(32, 32, 8, 3).obs_shape[1:]``), E = 65 536 envs, capacity 16, for
B in {64, 4 096, 65 536} and n_frames in {1, 4}; and a uint8 ``TurnBuffer`` of the same window at B = 65 536.  Three paths, timed in one
process with device events around every call, alternating call by call after a warm-up:

  torch    ``Buffer._sample_torch`` -- the indexing path (for the TurnBuffer: the same formula over ``agent_view`` + ``.float()``)
  host     ``Buffer.sample`` / ``TurnBuffer.sample`` with the same host-side index tensors: one upload + one ``sgw_sample`` launch
  device   ``ReplaySampler.sample()``: indices drawn by the kernel, nothing crosses the bus

The torch path is the baseline, and it is timed TWICE per round (torch, host, torch again, device): the difference between the medians
of its two series is the spread a difference between paths has to exceed.  Before any timing the outputs of the paths are compared on
the timed, seeded indices (the device-drawn batch against the torch path at ``last_index``).  Bytes moved per sample:
(n_frames + 1) rows read + 2 n_frames rows written (+ the scalars)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import torch  # noqa: E402
from _timing import Emitter, series, stats  # noqa: E402  (tools/_timing.py)

from sorrel_amd.buffers import Buffer, ReplaySampler, TurnBuffer, _stack_torch  # noqa: E402
from sorrel_amd.spec import treasurehunt_spec  # noqa: E402


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def report(emit, name, B, F, R, src_bytes, paths, reps):
    t_a, t_host, t_b, t_dev = series(paths, reps, warm=10)
    (ma, la, ha), (mb, lb, hb) = stats(t_a), stats(t_b)
    (mh, lh, hh), (md, ld, hd) = stats(t_host), stats(t_dev)
    base, spread = (ma + mb) / 2, abs(ma - mb)
    moved = B * ((F + 1) * R * src_bytes + 2 * F * R * 4 + 8 + 12 + 4 * F)
    emit(f"{name:10s} B={B:6d} n_frames={F}  torch {ma:9.1f} / {mb:9.1f} us (p10 {min(la, lb):.1f}, p90 {max(ha, hb):.1f}; spread of the medians {spread:.1f})")
    emit(f"{'':10s} host-drawn   sgw_sample {mh:9.1f} us (p10 {lh:.1f}, p90 {hh:.1f})  x{base / mh:6.2f}  {'faster' if base - mh > spread else 'NOT faster'} than torch by more than the spread")
    emit(f"{'':10s} device-drawn sgw_sample {md:9.1f} us (p10 {ld:.1f}, p90 {hd:.1f})  x{base / md:6.2f}  {'faster' if base - md > spread else 'NOT faster'}; "
         f"{moved / 1e6:.1f} MB moved -> {moved / md / 1e6:.2f} TB/s over the call's time")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--capacity", type=int, default=16)
    ap.add_argument("--batches", type=int, nargs="*", default=[64, 4096, 65536])
    ap.add_argument("--frames", type=int, nargs="*", default=[1, 4], help="n_frames values (one value: a kernel trace of the run shows one shape per kernel name)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sample needs a HIP device")
    emit = Emitter(args.out)

    dev = "cuda:0"
    window = tuple(treasurehunt_spec(32, 32, 8, 3).obs_shape[1:])
    R = 1
    for s in window:
        R *= s
    E, cap = args.envs, args.capacity
    emit(f"# tools/bench_sample.py --reps {args.reps} --envs {E} --capacity {cap}: {torch.cuda.get_device_name(0)}; window {window} = {R} elements; "
         f"microseconds per call, device events around each call, paths alternating call by call")
    gen = torch.Generator().manual_seed(1)          # the timed indices
    torch.manual_seed(2)                            # the rings' contents
    for F in args.frames:
        buf = Buffer(cap, window, n_frames=F, num_envs=E, device=dev)
        buf.states.copy_(torch.randint(0, 7, buf.states.shape, dtype=torch.uint8, device=dev))       # (filled on the device, from its seeded generator)
        buf.actions.copy_(torch.randint(0, 5, buf.actions.shape, device=dev))
        buf.rewards.copy_(torch.randint(-9, 10, buf.rewards.shape, device=dev).float())
        buf.dones.copy_((torch.rand(buf.dones.shape, device=dev) < 0.05).float())
        buf.idx, buf.size = 0, cap
        hi = max(1, cap - F - 1)
        for B in args.batches:
            t0, e = torch.randint(0, hi, (B,), generator=gen), torch.randint(0, E, (B,), generator=gen)
            sampler = ReplaySampler(buf, B, seed=7)
            want = buf._sample_torch(B, t0, e)
            if not same(buf.sample(B, t0, e), want):
                raise SystemExit(f"B={B} n_frames={F}: Buffer.sample differs from the torch path")
            drawn = [t.clone() for t in sampler.sample()]
            li = sampler.last_index.cpu()
            if not same(drawn, buf._sample_torch(B, li[:, 0], li[:, 1])):
                raise SystemExit(f"B={B} n_frames={F}: the device-drawn batch differs from the torch path at last_index")
            del want, drawn
            torch_path = lambda: buf._sample_torch(B, t0, e)     # noqa: E731
            report(emit, "Buffer f32", B, F, R, 4, (torch_path, lambda: buf.sample(B, t0, e), torch_path, sampler.sample), args.reps)
            del sampler
        del buf
        torch.cuda.empty_cache()
    A = 8
    B = args.batches[-1]
    for F in args.frames:
        ring = TurnBuffer(cap, E, (A, *window), device=dev, obs_dtype=torch.uint8)
        for lo in range(cap):
            ring.obs[lo].copy_(torch.randint(0, 256, ring.obs[lo].shape, dtype=torch.uint8, device=dev))
        ring.actions.copy_(torch.randint(0, 5, ring.actions.shape, dtype=torch.uint8, device=dev))
        ring.rewards.copy_(torch.randint(-9, 10, ring.rewards.shape, device=dev).float())
        ring.advance(cap)
        hi = max(1, cap - F - 1)
        t0, e = torch.randint(0, hi, (B,), generator=gen), torch.randint(0, E, (B,), generator=gen)

        def by_hand(t0=t0, e=e, F=F):
            s, a, r, ns, d, v = _stack_torch(*ring.agent_view(3), F, B, t0, e)
            return s.float(), a.long(), r, ns.float(), d, v

        sampler = ReplaySampler(ring, B, n_frames=F, agent=3, seed=7)
        if not same(ring.sample(B, agent=3, n_frames=F, starts=t0, envs=e), by_hand()):
            raise SystemExit(f"TurnBuffer n_frames={F}: TurnBuffer.sample differs from the torch path")
        drawn = [t.clone() for t in sampler.sample()]
        li = sampler.last_index.cpu()
        if not same(drawn, by_hand(li[:, 0], li[:, 1])):
            raise SystemExit(f"TurnBuffer n_frames={F}: the device-drawn batch differs from the torch path at last_index")
        del drawn
        report(emit, "TurnBuf u8", B, F, R, 1, (by_hand, lambda: ring.sample(B, agent=3, n_frames=F, starts=t0, envs=e), by_hand, sampler.sample), args.reps)
        del ring, sampler
        torch.cuda.empty_cache()
    emit.close()


if __name__ == "__main__":
    main()
