#!/usr/bin/env python3
"""Sampling a batch of action distributions on the device: ``sgw_policy_sample`` against the torch path it replaces
(``Categorical(probs, validate_args=False)``, ``.sample()``, ``.log_prob()``, ``.entropy()`` and the copy of the log-probabilities into a
ring row), and a whole policy turn through the Python API with either inside.  Prints the text of profiles/policy_sample.txt.

usage: python tools/bench_policy_sample.py [--reps 200] [--envs 65536 1024] [--turns 60] [--rounds 5] [--out FILE]

Part 1, the launch.  float32 rows of 4 and 16 actions at every ``--envs``, and 256 actions (the generic loop) once at the first.  Both
paths are timed in one process with device events around every call and alternate call by call after a warm-up: torch, kernel, torch
again.  The torch path is the baseline and is therefore timed TWICE per round: the difference between the medians of its two series is the
spread a difference between paths has to exceed.  Before any timing the outputs are compared on the timed data: the two paths draw from
different generators, so the kernel's actions are checked for what they are -- every one has a positive weight, and the counts of each
action lie within 6 binomial standard deviations of the sum of its probabilities -- and its log-probabilities and entropies are compared
with ``Categorical`` over the same rows in float64 (``.log_prob`` of the kernel's actions, ``.entropy``), rounded to float32: at most one
ulp apart.  Algorithmic bytes per row: ``4 n_actions`` read + 8 + 4 + 4 written.

Part 2, the turn.  Treasurehunt 32x32, 8 agents, 7x7 windows, 1 024 envs, a one-layer softmax policy per agent: ``take_action`` either
samples with torch's ``Categorical`` (and copies the log-probabilities into a ring row itself) or returns ``ActionProbs``; eager (the fast
policy loop) and recorded (``capture_turn(force=True)``).  Wall time per turn over ``--turns`` turns ending in a device synchronise,
``--rounds`` rounds alternating torch, ActionProbs, torch."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
from _timing import Emitter, series, stats  # noqa: E402  (tools/_timing.py)
from torch.distributions import Categorical  # noqa: E402

from sorrel_amd import _native as N  # noqa: E402


def ulps(a, b):
    def ordered(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(np.asarray(a, np.float32)) - ordered(np.asarray(b, np.float32)))


def launch_case(E, na, reps, emit):
    dev = "cuda:0"
    lib = N.load()
    probs = torch.softmax(torch.randn((E, na), device=dev) * 1.5, dim=1)
    ring = torch.zeros((4, E), dtype=torch.float32, device=dev)
    acts = torch.zeros((E,), dtype=torch.int64, device=dev)
    ent = torch.zeros((E,), dtype=torch.float32, device=dev)
    d = N.SgwPolicyDesc()
    d.dist, d.out_actions, d.out_log_probs, d.out_entropy = probs.data_ptr(), acts.data_ptr(), ring[1].data_ptr(), ent.data_ptr()
    d.n, d.num_envs, d.row_stride, d.num_actions = E, E, na, na
    d.seed, d.epoch, d.turn, d.agent0 = 12345, 1, 1, 2
    d.dist_type, d.mode = N.POLICY_F32, N.POLICY_PROBS
    turn = [0]

    def kernel():
        turn[0] += 1
        d.turn = turn[0]                       # (another draw every call, as in a turn loop)
        N.check(lib.sgw_policy_sample(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    tout = {}

    def by_torch():
        dist = Categorical(probs=probs, validate_args=False)
        a = dist.sample()
        ring[2].copy_(dist.log_prob(a))
        tout["a"], tout["ent"] = a, dist.entropy()

    kernel()
    torch.cuda.synchronize()
    p64 = probs.double()
    ref = Categorical(probs=p64, validate_args=False)
    a_host = acts.cpu().numpy()
    assert (probs.cpu().numpy()[np.arange(E), a_host] > 0).all(), "an action of weight zero was chosen"
    counts = np.bincount(a_host, minlength=na)
    q = (p64 / p64.sum(dim=1, keepdim=True)).cpu().numpy()
    mean, sd = q.sum(axis=0), np.sqrt((q * (1 - q)).sum(axis=0))
    dev_sd = float((np.abs(counts - mean) / np.maximum(sd, 1e-9)).max())
    if dev_sd > 6:
        raise SystemExit(f"E={E} n_actions={na}: an action's count lies {dev_sd:.1f} standard deviations from the sum of its probabilities")
    u_lp = int(ulps(ring[1].cpu().numpy(), ref.log_prob(acts).float().cpu().numpy()).max())
    u_en = int(ulps(ent.cpu().numpy(), ref.entropy().float().cpu().numpy()).max())
    if u_lp > 1 or u_en > 1:
        raise SystemExit(f"E={E} n_actions={na}: log-probabilities {u_lp} ulp, entropies {u_en} ulp from Categorical in float64")
    verdict = f"counts within {dev_sd:.2f} sd; log-prob {u_lp} ulp, entropy {u_en} ulp from float64 Categorical"
    t_a, t_k, t_b = series((by_torch, kernel, by_torch), reps, warm=5)
    (ma, la, ha), (mb, lb, hb), (mk, lk, hk) = stats(t_a), stats(t_b), stats(t_k)
    base, spread = (ma + mb) / 2, abs(ma - mb)
    moved = E * (4 * na + 16)
    name = f"E={E} n_actions={na} float32"
    emit(f"{name:34s} torch Categorical {ma:9.1f} / {mb:9.1f} us (p10 {min(la, lb):.1f}, p90 {max(ha, hb):.1f}; spread of the medians {spread:.1f})")
    emit(f"{'':34s} sgw_policy_sample {mk:9.1f} us (p10 {lk:.1f}, p90 {hk:.1f})  x{base / mk:7.2f}  {'faster' if base - mk > spread else 'NOT faster'} than torch by more "
         f"than the spread; {moved / 1e6:.2f} MB algorithmic -> {moved / mk / 1e6:.3f} TB/s over the call's time (HBM peak 8 TB/s); {verdict}")


def make_env(kind, E, agents=8):
    from sorrel_amd.buffers import Buffer, RolloutBuffer
    from sorrel_amd.examples.treasurehunt.entities import EmptyEntity
    from sorrel_amd.examples.treasurehunt.env import TreasurehuntEnv
    from sorrel_amd.examples.treasurehunt.main import make_config
    from sorrel_amd.examples.treasurehunt.world import TreasurehuntWorld
    from sorrel_amd.models import ActionProbs, BaseModel

    dev = "cuda:0"

    class Softmax(BaseModel):
        def __init__(self, input_size, action_space, k):
            super().__init__(input_size, action_space, memory_size=0, num_envs=E, device=dev)
            ring = RolloutBuffer if kind == "probs" else Buffer
            self.memory = ring(capacity=64, obs_shape=tuple(input_size), num_envs=E, device=dev)
            self.lp_row = torch.zeros((E,), dtype=torch.float32, device=dev)
            g = torch.Generator().manual_seed(k)
            self.weight = (torch.randn((int(np.prod(input_size)), action_space), generator=g) * 0.3).to(dev)

        def take_action(self, state):
            probs = torch.softmax(state @ self.weight, dim=1)
            if kind == "probs":
                return ActionProbs(probs)
            dist = Categorical(probs=probs, validate_args=False)
            a = dist.sample()
            self.lp_row.copy_(dist.log_prob(a))
            return a

    made = []

    def factory(input_size, action_space):
        made.append(Softmax(input_size, action_space, len(made)))
        return made[-1]

    cfg = make_config(32, 32, agents, 3, spawn_prob=0.02, max_turns=1 << 30)
    world = TreasurehuntWorld(cfg, EmptyEntity(), num_envs=E, device=dev, seed=5)
    return TreasurehuntEnv(world, cfg, model_factory=factory)


def turn_case(recorded, turns, rounds, emit):
    E = 1024
    envs = {kind: make_env(kind, E) for kind in ("torch", "probs")}
    note = {}
    for kind, env in envs.items():
        if recorded:
            cap = env.capture_turn(warmup=2, force=True)
            note[kind] = "recorded" if cap is not None else f"NOT recordable ({type(env.capture_error).__name__}: {str(env.capture_error)[:80]}): the eager loop plays"
        else:
            note[kind] = "eager, " + env.turn_plan()["loop"] + " loop"
        for _ in range(10):
            env.take_turn()
    torch.cuda.synchronize()

    def run(env):
        t0 = time.perf_counter()
        for _ in range(turns):
            env.take_turn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / turns * 1e6

    t_a, t_k, t_b = [], [], []
    for _ in range(rounds):
        t_a.append(run(envs["torch"]))
        t_k.append(run(envs["probs"]))
        t_b.append(run(envs["torch"]))
    ma, mb, mk = statistics.median(t_a), statistics.median(t_b), statistics.median(t_k)
    base, spread = (ma + mb) / 2, abs(ma - mb)
    name = f"turn, 8 agents x {E} envs, {'recorded' if recorded else 'eager'}"
    emit(f"{name:34s} torch Categorical in take_action {ma:8.1f} / {mb:8.1f} us per turn (min {min(t_a + t_b):.1f}, max {max(t_a + t_b):.1f}; spread of the medians {spread:.1f}) [{note['torch']}]")
    emit(f"{'':34s} ActionProbs                      {mk:8.1f} us per turn (min {min(t_k):.1f}, max {max(t_k):.1f})  x{base / mk:6.2f}  "
         f"{'faster' if base - mk > spread else 'NOT faster'} than the torch path by more than the spread [{note['probs']}]")
    for env in envs.values():
        env.raise_on_status()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--envs", type=int, nargs="*", default=[65536, 1024])
    ap.add_argument("--turns", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_sample needs a HIP device")
    emit = Emitter(args.out, as_it_grows=True)          # (kept as it grows: a later case that fails leaves the earlier lines)

    emit(f"# tools/bench_policy_sample.py --reps {args.reps} --envs {' '.join(map(str, args.envs))} --turns {args.turns} --rounds {args.rounds}: "
         f"{torch.cuda.get_device_name(0)}; launches: microseconds per call, device events around each call, paths alternating call by call "
         f"(torch, kernel, torch); turns: wall microseconds per turn, blocks of {args.turns} turns ending in a synchronise, alternating (torch, ActionProbs, torch)")
    torch.manual_seed(3)
    for E in args.envs:
        for na in (4, 16):
            launch_case(E, na, args.reps, emit)
    launch_case(args.envs[0], 256, args.reps, emit)
    turn_case(False, args.turns, args.rounds, emit)
    turn_case(True, args.turns, args.rounds, emit)


if __name__ == "__main__":
    main()
