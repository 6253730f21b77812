#!/usr/bin/env python3
"""Adam, gradient clipping and the soft update on the device: ``sgw_adam_step`` (through ``sorrel_amd.optim.FusedAdam``) against the
reference's lines on device tensors (``sorrel_amd.optim._adam_step_torch``).  Prints the text of profiles/adam_step.txt.

usage: python tools/bench_adam_step.py [--reps 20] [--out FILE]

Shapes: the parameter list of the reference's IQN as the Treasurehunt example configures it (16 float32 tensors: a 6 x 5 x 5 window,
5 frames, 250 units, 4 actions; clip 1, soft update); PPO's ``ActorCritic`` (16 float64 tensors, two groups with learning rates of
their own; no clipping, no targets); 64 tensors of 2^20 float32 (clip 1, soft update), reported as bytes over time too.

Baselines, both the reference's lines: ``clip_grad_norm_``, the optimiser's step, the ``soft_update`` loop -- once with torch's default
``Adam`` and that loop as written, once with ``Adam(fused=True)`` and ``torch._foreach_mul_`` / ``_foreach_add_`` for the soft update,
the strongest torch form.  All paths run in one process with device events around every call and alternate call by call after a
warm-up: default, fused, kernel, default, fused -- so both baselines are timed before AND after the kernel's series, and the
difference between a baseline's two medians is the spread a difference between paths has to exceed.  Before any timing one step of
every path from the same start is compared: parameters, moments and targets to 2^-18 of each tensor's largest magnitude (the tests
hold the real formulas).  Algorithmic bytes of the third shape: ``4 N`` read for the norm plus ``(5 + 4) 4 N`` for
the update."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import torch  # noqa: E402
from _timing import Emitter, one, stats  # noqa: E402  (tools/_timing.py)

from sorrel_amd import optim  # noqa: E402


def iqn_shapes(inputs=6 * 5 * 5, frames=5, units=250, actions=4, n_cos=64):
    noisy = lambda o, i: [(o, i), (o,), (o, i), (o,)]      # noqa: E731  (weight, bias, sigma_weight, sigma_bias)
    return [(units, frames * inputs), (units,), (units, n_cos), (units,)] + noisy(units, units) + noisy(actions, units) + noisy(1, units)


def actor_critic_shapes(inputs=6 * 5 * 5, units=64, actions=4):
    net = lambda out: [(units, inputs), (units,), (2 * units, units), (2 * units,), (units, 2 * units), (units,), (out, units), (out,)]  # noqa: E731
    return net(actions), net(1)


class Case:
    """One parameter list in three copies (default torch, fused torch, kernel) that start from the same values and see the same gradients."""

    def __init__(self, groups, dtype, clip, tau, dev):
        self.clip, self.tau = clip, tau
        gen = torch.Generator(device=dev).manual_seed(7)
        start = [[torch.randn(s, device=dev, dtype=dtype, generator=gen) * 0.1 for s in shapes] for shapes, _ in groups]
        self.grads = [torch.randn(s, device=dev, dtype=dtype, generator=gen) * 0.05 for shapes, _ in groups for s in shapes]
        self.sets = []
        for _ in range(3):
            params = [[torch.nn.Parameter(x.clone()) for x in g] for g in start]
            flat = [p for g in params for p in g]
            for p, g in zip(flat, self.grads):
                p.grad = g.clone()
            targets = [torch.zeros_like(p) for p in flat] if tau is not None else None
            self.sets.append((params, flat, targets))
        lrs = [lr for _, lr in groups]
        as_groups = lambda params: [dict(params=g, lr=lr) for g, lr in zip(params, lrs)]      # noqa: E731
        self.opt_default = torch.optim.Adam(as_groups(self.sets[0][0]))
        self.opt_fused = torch.optim.Adam(as_groups(self.sets[1][0]), fused=True)
        self.opt_kernel = optim.FusedAdam(as_groups(self.sets[2][0]), max_grad_norm=clip, target_params=self.sets[2][2], tau=tau)
        self.numel = sum(p.numel() for p in self.sets[0][1])

    def regrad(self, flat):
        # clip_grad_norm_ scales the gradients in place: put the same ones back before every torch call (outside the timed region)
        for p, g in zip(flat, self.grads):
            p.grad.copy_(g)

    def default(self):
        _, flat, targets = self.sets[0]
        optim._adam_step_torch(flat, self.opt_default, self.clip, targets, self.tau)

    def fused(self):
        _, flat, targets = self.sets[1]
        if self.clip is not None:
            torch.nn.utils.clip_grad_norm_(flat, self.clip)
        self.opt_fused.step()
        if targets is not None:
            data = [p.data for p in flat]
            torch._foreach_mul_(targets, 1.0 - self.tau)
            torch._foreach_add_(targets, data, alpha=self.tau)

    def kernel(self):
        self.opt_kernel.step()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adam_step needs a HIP device")
    emit = Emitter(args.out)

    dev = torch.device("cuda:0")
    emit(f"# tools/bench_adam_step.py --reps {args.reps}: {torch.cuda.get_device_name(0)}; microseconds per call, device events around each call, "
         f"paths alternating call by call (default, fused, kernel, default, fused)")
    actor, critic = actor_critic_shapes()
    cases = (("IQN Treasurehunt, 16 float32 tensors, clip 1, soft update", [(iqn_shapes(), 1e-3)], torch.float32, 1.0, 0.001),
             ("PPO ActorCritic, 16 float64 tensors, two groups", [(actor, 3e-4), (critic, 1e-3)], torch.float64, None, None),
             ("64 tensors of 2^20 float32, clip 1, soft update", [([(1 << 20,)] * 64, 1e-3)], torch.float32, 1.0, 0.001))
    for name, groups, dtype, clip, tau in cases:
        case = Case(groups, dtype, clip, tau, dev)
        # one step of every path from the same start, compared
        case.default(), case.fused(), case.kernel()
        torch.cuda.synchronize()
        worst = dict(param=0.0, exp_avg=0.0, exp_avg_sq=0.0, target=0.0)
        for other, opt in ((0, case.opt_default), (1, case.opt_fused)):
            for k, (p, q) in enumerate(zip(case.sets[other][1], case.sets[2][1])):
                pairs = [("param", p.detach(), q.detach())] + [(key, opt.state[p][key], case.opt_kernel.state[q][key]) for key in ("exp_avg", "exp_avg_sq")]
                if tau is not None:
                    pairs.append(("target", case.sets[other][2][k], case.sets[2][2][k]))
                for key, a, b in pairs:
                    worst[key] = max(worst[key], float((a - b).abs().max() / a.abs().max()))
        if max(worst.values()) > 2.0 ** -18:
            raise SystemExit(f"{name}: sgw_adam_step differs from the torch paths: {worst}")
        torch_sets = (case.sets[0][1], case.sets[1][1])
        fns = ((case.default, torch_sets[0]), (case.fused, torch_sets[1]), (case.kernel, None), (case.default, torch_sets[0]), (case.fused, torch_sets[1]))

        def call(fn, flat, timed):
            if flat is not None and clip is not None:       # (outside the timed region)
                case.regrad(flat)
                torch.cuda.synchronize()
            return one(fn) if timed else fn()

        for _ in range(3):
            for fn, flat in fns:
                call(fn, flat, False)
        torch.cuda.synchronize()
        out = [[] for _ in fns]
        for _ in range(args.reps):
            for (fn, flat), o in zip(fns, out):
                o.append(call(fn, flat, True))
        (d0, d0l, d0h), (f0, f0l, f0h), (k, kl, kh), (d1, d1l, d1h), (f1, f1l, f1h) = (stats(o) for o in out)
        emit(f"{name}: {case.numel} elements; first steps agree: moments to {max(worst['exp_avg'], worst['exp_avg_sq']):.2e}, "
             f"params to {worst['param']:.2e}, targets to {worst['target']:.2e} of the largest magnitude")
        emit(f"    torch default Adam      {d0:10.1f} / {d1:10.1f} us (p10 {min(d0l, d1l):.1f}, p90 {max(d0h, d1h):.1f}; spread of the medians {abs(d0 - d1):.1f})")
        emit(f"    torch Adam(fused=True)  {f0:10.1f} / {f1:10.1f} us (p10 {min(f0l, f1l):.1f}, p90 {max(f0h, f1h):.1f}; spread of the medians {abs(f0 - f1):.1f})")
        line = f"    sgw_adam_step           {k:10.1f} us (p10 {kl:.1f}, p90 {kh:.1f})  x{(d0 + d1) / 2 / k:7.2f} against default, x{(f0 + f1) / 2 / k:7.2f} against fused"
        if case.numel >= 1 << 26:
            moved = (4 if clip is not None else 0) * case.numel + (5 + 4) * 4 * case.numel
            line += f"; {moved / 1e6:.1f} MB algorithmic -> {moved / k / 1e6:.3f} TB/s over the call's time (HBM peak 8 TB/s)"
        emit(line)
        del case
        torch.cuda.empty_cache()
    emit.close()


if __name__ == "__main__":
    main()
