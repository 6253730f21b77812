#!/usr/bin/env python3
"""A whole IQN learner step four ways.  Prints the text of profiles/iqn_learner.txt (profiles/iqn_learner_recorded.txt since the recorded column).

usage: python tools/bench_iqn_learner.py [--reps 20] [--out FILE]
       python tools/bench_iqn_learner.py --only device|recorded|hand|torch --batch 64 --steps 10      (one path alone, for a kernel trace)
       python tools/bench_iqn_learner.py --sum-calls DIR                                       (total of the Calls column of a trace's *kernel_stats.csv)

The reference's shape (in_features 875, layer_size 250, 12 quantiles, 4 actions), batches of 64 (the reference's), 1 024 and 4 096 states
sampled from a replay ring of twice the batch; the reference's hyper-parameters.  The paths:

* ``device``: ``PyTorchIQN.train_step()`` on the device (sgw_sample, sgw_noisy_weights, 3 x sgw_iqn_forward, sgw_iqn_loss, sgw_iqn_backward,
  sgw_noisy_weights backwards, sgw_adam_step, one copy of the loss).  It is the BASELINE of the recorded path (the same code before and
  after that path existed) and is timed in two series per round, so that its own spread is known;
* ``recorded``: the same step after ``capture_train_step()``: one graph replay (the clocked twins of the three calls that take the step's count
  or the ring's filled rows, ``sgw_learn_clock_advance`` last);
* ``hand``: the hand-written step of ``sorrel_amd/losses.py``'s docstring from public calls (``Buffer.sample``, ``IQN.quantiles`` x 2,
  ``IQN.forward_fused``, ``iqn_loss``, ``backward()``, ``FusedAdam.step()``): what the package offered before the learner class, and the
  BASELINE: it is timed twice per round, and the difference of its two medians is the spread a difference between paths has to exceed;
* ``torch``: ``Buffer.sample``, ``IQN.forward`` x 3 with autograd, the loss as torch ops, ``clip_grad_norm_``, ``torch.optim.Adam`` and the
  soft-update loop.

One process; device events around each step; after a warm-up the paths alternate step by step and the order is reversed every other round.
Each path owns its networks and optimiser (same start).  Behind the event times: wall time per step over ``--wall`` back-to-back steps of
the eager and the recorded ``train_step`` (one synchronisation at the end), which is where host time shows.  Nothing is asserted about
speed; the numbers are reported as they come.  The
launch counts per step come from a kernel trace of each path alone (``--only``), taken as the difference of two runs of different length."""
import argparse
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

OBS, L, NQ, A = 875, 250, 12, 4
BATCHES = (64, 1024, 4096)
HYPER = dict(LR=0.001, TAU=0.001, GAMMA=0.99, n_step=3)


def sum_calls(directory):
    total, files = 0, sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    for path in files:
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                total += int(row["Calls"])
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {directory}")
    return total


def make_paths(B, dev):
    import torch
    from torch.nn.utils import clip_grad_norm_

    from sorrel_amd.losses import _iqn_loss_torch, iqn_loss
    from sorrel_amd.models import PyTorchIQN
    from sorrel_amd.models.iqn import IQN
    from sorrel_amd.optim import FusedAdam

    def learner():
        m = PyTorchIQN((OBS,), A, L, 0.0, dev, 5, n_frames=1, batch_size=B, memory_size=2 * B, n_quantiles=NQ, **HYPER)
        g = torch.Generator().manual_seed(9)
        m.memory.states.copy_(torch.randn(m.memory.states.shape, generator=g))
        m.memory.actions.copy_(torch.randint(0, A, m.memory.actions.shape, generator=g))
        m.memory.rewards.copy_(torch.randn(m.memory.rewards.shape, generator=g))
        m.memory.size = m.memory.capacity
        return m

    device_model = learner()
    discount = HYPER["GAMMA"] ** HYPER["n_step"]

    hand = learner()
    h_local, h_target, h_mem = hand.qnetwork_local, hand.qnetwork_target, hand.memory
    h_opt = FusedAdam(h_local.parameters(), lr=HYPER["LR"], max_grad_norm=1, target_params=h_target.parameters(), tau=HYPER["TAU"])

    def by_hand():
        states, actions, rewards, next_states, dones, valid = h_mem.sample(B)
        q_next_local = h_local.quantiles(next_states).quantiles
        q_next_target = h_target.quantiles(next_states).quantiles
        q_expected, taus = h_local.forward_fused(states)
        loss = iqn_loss(q_expected, taus, q_next_local, q_next_target, actions, rewards, dones, valid, discount)
        h_opt.zero_grad(set_to_none=True)
        loss.backward()
        h_opt.step()
        return loss

    plain = learner()
    t_local, t_target, t_mem = plain.qnetwork_local, plain.qnetwork_target, plain.memory
    t_opt = torch.optim.Adam(t_local.parameters(), lr=HYPER["LR"])
    assert isinstance(t_local, IQN)

    def by_torch():
        t_opt.zero_grad()
        states, actions, rewards, next_states, dones, valid = t_mem.sample(B)
        q_next_local, _ = t_local(next_states, NQ)
        q_next_target, _ = t_target(next_states, NQ)
        q_expected, taus = t_local(states, NQ)
        loss = _iqn_loss_torch(q_expected, taus, q_next_local, q_next_target, actions, rewards, dones, valid, discount)[0]
        loss.backward()
        clip_grad_norm_(t_local.parameters(), 1)
        t_opt.step()
        for target_param, local_param in zip(t_target.parameters(), t_local.parameters()):
            target_param.data.copy_(HYPER["TAU"] * local_param.data + (1.0 - HYPER["TAU"]) * target_param.data)
        return loss

    recorded_model = learner()
    recorded_model.capture_train_step(warmup=2)

    return dict(device=device_model.train_step, recorded=recorded_model.train_step, hand=by_hand, torch=by_torch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("device", "recorded", "hand", "torch"), default=None)
    ap.add_argument("--wall", type=int, default=200)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--sum-calls", default=None)
    args = ap.parse_args()
    if args.sum_calls:
        print(sum_calls(args.sum_calls))
        return
    import torch
    from _timing import Emitter, one, stats  # (tools/_timing.py)

    if not torch.cuda.is_available():
        raise SystemExit("bench_iqn_learner needs a HIP device")
    dev = torch.device("cuda:0")
    if args.only:
        step = make_paths(args.batch, dev)[args.only]
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        print(f"{args.only}: {args.steps} steps at B={args.batch}")
        return
    emit = Emitter(args.out, as_it_grows=True)
    emit(f"# tools/bench_iqn_learner.py --reps {args.reps}: {torch.cuda.get_device_name(0)}; in_features {OBS}, layer_size {L}, {NQ} quantiles, {A} actions; "
         f"microseconds per learner step (sampling the batch included), device events around each step, paths alternating step by step "
         f"(hand, device, recorded, torch, device, hand; the order reversed every other round); wall time per step over {args.wall} back-to-back steps")
    import time

    for B in BATCHES:
        paths = make_paths(B, dev)
        order = [("hand", paths["hand"]), ("device", paths["device"]), ("recorded", paths["recorded"]), ("torch", paths["torch"]),
                 ("device2", paths["device"]), ("hand2", paths["hand"])]
        for _ in range(3):
            for _, f in order:
                f()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in order}
        for r in range(args.reps):
            for name, f in (order if r % 2 == 0 else order[::-1]):
                times[name].append(one(f))
        (m1, lo1, hi1), (m2, _, _) = stats(times["hand"]), stats(times["hand2"])
        (md, lod, hid), (mt, lot, hit) = stats(times["device"]), stats(times["torch"])
        (md2, _, _), (mr, lor, hir) = stats(times["device2"]), stats(times["recorded"])
        spread, base = abs(m1 - m2), 0.5 * (m1 + m2)
        dspread, dbase = abs(md - md2), 0.5 * (md + md2)

        def verdict(m):
            return ("faster than the hand-written step by more than the spread" if m < base - spread else
                    "SLOWER than the hand-written step by more than the spread" if m > base + spread else "within the spread of the hand-written step")

        emit(f"B={B:<5} hand-written step   {m1:9.1f} / {m2:9.1f} us (p10 {lo1:.1f}, p90 {hi1:.1f}; spread of the medians {spread:.1f})")
        emit(f"{'':8}train_step (device) {md:9.1f} / {md2:9.1f} us (p10 {lod:.1f}, p90 {hid:.1f}; spread of the medians {dspread:.1f})  x {base / md:6.2f}  {verdict(md)}")
        emit(f"{'':8}train_step recorded {mr:9.1f} us (p10 {lor:.1f}, p90 {hir:.1f})  x {dbase / mr:6.2f} of the eager train_step: " +
             ("faster by more than its spread" if mr < dbase - dspread else "SLOWER by more than its spread" if mr > dbase + dspread else "within its spread"))
        emit(f"{'':8}all-torch step      {mt:9.1f} us (p10 {lot:.1f}, p90 {hit:.1f})  x {base / mt:6.2f}  {verdict(mt)}")
        wall = {}
        for name in ("device", "recorded", "device2"):
            f = paths[name.rstrip("2")]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.wall):
                f()
            torch.cuda.synchronize()
            wall[name] = (time.perf_counter() - t0) * 1e6 / args.wall
        emit(f"{'':8}wall per step, {args.wall} back to back: eager {wall['device']:.1f} / {wall['device2']:.1f} us, recorded {wall['recorded']:.1f} us "
             f"(x {0.5 * (wall['device'] + wall['device2']) / wall['recorded']:.2f})")
    emit.close()


if __name__ == "__main__":
    main()
