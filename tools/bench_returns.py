#!/usr/bin/env python3
"""Discounted returns on the device: ``sgw_returns`` against the torch path it replaces (``sorrel_amd.buffers._returns_torch``: a loop over
the turns, a handful of launches each).  Prints the text of profiles/returns.txt.

usage: python tools/bench_returns.py [--reps 30] [--turns 100] [--envs 65536 1024] [--out FILE]

Rings: a ``TurnBuffer`` of T = 100 turns, A = 8 agents and E = 65 536 envs (the config-3 ring) read over every (env, agent) column
(``agent=None``) and over one agent's (``agent=3``, column stride A); the same with E = 1 024 (few columns: latency, not bandwidth);
and a ``Buffer`` of T = 100, E = 65 536.  Each with ``normalize`` None / "column" / "all" (float64 normalised values).

Both paths write into storage made before the timing (``out=``), are timed in one process with device events around every call, and
alternate call by call after a warm-up: torch, kernel, torch again.  The torch path is the baseline and is therefore timed TWICE per
round: the difference between the medians of its two series is the spread a difference between paths has to exceed.  Before any timing
the outputs are compared on the timed data: raw returns for equality, normalised values against the torch path's within the tolerance
of the tests, ``8 T 2^-53 (1 + max|x| / (std + 1e-7))``.  Algorithmic bytes per element: 8 read + 4 written, + 4 re-read + 8 written with
normalisation."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import torch  # noqa: E402
from _timing import Emitter, series, stats  # noqa: E402  (tools/_timing.py)

from sorrel_amd.buffers import Buffer, TurnBuffer, _returns_torch, _returns_views  # noqa: E402

GAMMA = 0.99


def fill(ring):
    """Rewards that are multiples of float32(0.37), dones on 2 % of the slots: filled on the device from its seeded generator."""
    ring.rewards.copy_(torch.randint(-10, 11, ring.rewards.shape, device=ring.device).float() * 0.37)
    ring.dones.copy_((torch.rand(ring.dones.shape, device=ring.device) < 0.02).float())
    ring.idx, ring.size = 0, ring.capacity


def compare(name, got, want, mode):
    if not torch.equal(got.returns, want.returns):
        raise SystemExit(f"{name}: sgw_returns differs from the torch path (raw returns)")
    if mode is None:
        return "raw returns equal"
    x = want.returns.double()
    T = x.shape[0] if mode == "column" else x.numel()
    dim = 0 if mode == "column" else None
    peak = x.abs().amax(dim=dim) if mode == "column" else x.abs().max()
    tol = 8 * T * 2.0 ** -53 * (1 + peak / (x.std(dim=dim) + 1e-7))
    err = (got.normalized - want.normalized).abs()
    share = float((err / tol).max())
    if not share <= 1.0:
        raise SystemExit(f"{name}: normalised values differ from the torch path's by {share:.3f} of the tolerance")
    return f"raw returns equal, normalised within {share:.4f} of the tolerance of the torch path's"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--turns", type=int, default=100)
    ap.add_argument("--agents", type=int, default=8)
    ap.add_argument("--envs", type=int, nargs="*", default=[65536, 1024])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_returns needs a HIP device")
    emit = Emitter(args.out)

    dev, T, A = "cuda:0", args.turns, args.agents
    emit(f"# tools/bench_returns.py --reps {args.reps} --turns {T} --agents {A} --envs {' '.join(map(str, args.envs))}: {torch.cuda.get_device_name(0)}; "
         f"gamma {GAMMA}; microseconds per call, device events around each call, paths alternating call by call (torch, kernel, torch)")
    torch.manual_seed(2)
    cases = []
    for E in args.envs:
        cases += [("TurnBuffer", E, None), ("TurnBuffer", E, 3)]
    cases.append(("Buffer", args.envs[0], None))
    for kind, E, agent in cases:
        ring = TurnBuffer(T, E, (A, 1, 1, 1), device=dev, obs_dtype=torch.uint8) if kind == "TurnBuffer" else Buffer(T, (1,), num_envs=E, device=dev)
        fill(ring)
        rewards, dones, _, _ = _returns_views(ring, agent)
        kw = dict(agent=agent) if kind == "TurnBuffer" else {}
        cols = rewards[0].numel()
        name = f"{kind} T={T} E={E}" + (f" A={A} agent={agent}" if kind == "TurnBuffer" else "")
        for mode in (None, "column", "all"):
            got = ring.returns(GAMMA, normalize=mode, **kw)
            want = _returns_torch(rewards, dones, GAMMA, 0, T, normalize=mode)
            torch.cuda.synchronize()
            verdict = compare(name, got, want, mode)
            kernel = lambda: ring.returns(GAMMA, normalize=mode, out=got, **kw)                      # noqa: E731
            by_torch = lambda: _returns_torch(rewards, dones, GAMMA, 0, T, normalize=mode, out=want)   # noqa: E731
            t_a, t_k, t_b = series((by_torch, kernel, by_torch), args.reps, warm=3)
            (ma, la, ha), (mb, lb, hb), (mk, lk, hk) = stats(t_a), stats(t_b), stats(t_k)
            base, spread = (ma + mb) / 2, abs(ma - mb)
            moved = T * cols * (12 if mode is None else 24)
            emit(f"{name:40s} normalize={str(mode):6s}  torch {ma:10.1f} / {mb:10.1f} us (p10 {min(la, lb):.1f}, p90 {max(ha, hb):.1f}; spread of the medians {spread:.1f})")
            emit(f"{'':40s} sgw_returns {mk:10.1f} us (p10 {lk:.1f}, p90 {hk:.1f})  x{base / mk:7.2f}  {'faster' if base - mk > spread else 'NOT faster'} than torch by more "
                 f"than the spread; {moved / 1e6:.1f} MB algorithmic -> {moved / mk / 1e6:.3f} TB/s over the call's time (HBM peak 8 TB/s); {verdict}")
            del got, want
        del ring, rewards, dones
        torch.cuda.empty_cache()
    emit.close()


if __name__ == "__main__":
    main()
