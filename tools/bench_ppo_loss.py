#!/usr/bin/env python3
"""PPO's clipped loss on the device: ``sgw_ppo_loss`` against the torch path it replaces (``sorrel_amd.losses._ppo_loss_torch``: the
reference's lines as torch ops, forward AND backward through autograd).  Prints the text of profiles/ppo_loss.txt.

usage: python tools/bench_ppo_loss.py [--reps 20] [--out FILE]

Shapes: a ring segment of T = 100 turns x E = 65 536 envs and of 100 x 1 024 (few rows: latency, not bandwidth) with 4 and 16 actions,
and 65 536 rows of 256 actions (the generic loop); float64 probabilities, values and returns, int64 actions, float32 stored
log-probabilities.  The stored log-probabilities are offset from the current ones so that ratios fall inside, above and below the clip
range.

Both paths are timed in one process with device events around every call and alternate call by call after a warm-up: torch, kernel,
the autograd wrapper, torch again.  The torch path is the baseline and is therefore timed TWICE per round: the difference between the
medians of its two series is the spread a difference between paths has to exceed.  ``kernel`` is ``ppo_loss_terms(out=)`` (two
launches, nothing allocated); ``wrapper`` is ``ppo_loss(out=).backward()`` on leaf tensors, i.e. the same two launches plus what
autograd adds: a clone of the scalar, the multiply of either saved gradient by the incoming gradient and the accumulation into
``.grad``.  Before any timing the outputs are compared on the timed data (the tests hold the tolerance formulas; here a coarse
2^-40 of the largest magnitude).  Algorithmic bytes per row: ``8 A`` read + ``8 A`` written for the distribution and its gradient,
8 + 8 + 8 + 4 read for value, action, return and stored log-probability, 8 written for the value's gradient."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import torch  # noqa: E402
from _timing import Emitter, series, stats  # noqa: E402  (tools/_timing.py)

from sorrel_amd import losses  # noqa: E402
from sorrel_amd.models import ActionProbs  # noqa: E402

EPS_CLIP, ENTROPY_COEF = 0.2, 0.01
SHAPES = ((100 * 65536, 4), (100 * 65536, 16), (100 * 1024, 4), (100 * 1024, 16), (65536, 256))


def batch(n, na, dev):
    probs = torch.softmax(torch.randn((n, na), dtype=torch.float64, device=dev), dim=-1)
    values = torch.randn((n,), dtype=torch.float64, device=dev)
    returns = torch.randn((n,), dtype=torch.float64, device=dev)
    actions = torch.randint(0, na, (n,), device=dev)
    now = torch.log(probs.gather(1, actions[:, None]).squeeze(1))
    target = 1.0 + torch.tensor([0.0, 2.0, -2.0, 0.5, 3.0, -0.5, -3.0], dtype=torch.float64, device=dev)[torch.arange(n, device=dev) % 7] * EPS_CLIP
    old = (now - torch.log(target)).float()
    return probs, values, actions, old, returns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ppo_loss needs a HIP device")
    emit = Emitter(args.out)

    dev = torch.device("cuda:0")
    emit(f"# tools/bench_ppo_loss.py --reps {args.reps}: {torch.cuda.get_device_name(0)}; eps_clip {EPS_CLIP}, entropy_coef {ENTROPY_COEF}; float64; "
         f"microseconds per call, device events around each call, paths alternating call by call (torch, kernel, wrapper, torch)")
    torch.manual_seed(3)
    for n, na in SHAPES:
        probs, values, actions, old, returns = batch(n, na, dev)
        res = losses.ppo_loss_terms(ActionProbs(probs), values, actions, old, returns, EPS_CLIP, ENTROPY_COEF)
        lp, lv = probs.clone().requires_grad_(True), values.clone().requires_grad_(True)

        def by_torch():
            lp.grad = lv.grad = None
            losses._ppo_loss_torch(lp, False, lv, actions, old, returns, EPS_CLIP, ENTROPY_COEF)[0].backward()

        def kernel():
            losses.ppo_loss_terms(ActionProbs(probs), values, actions, old, returns, EPS_CLIP, ENTROPY_COEF, out=res)

        kp, kv = probs.clone().requires_grad_(True), values.clone().requires_grad_(True)

        def wrapper():
            kp.grad = kv.grad = None
            losses.ppo_loss(ActionProbs(kp), kv, actions, old, returns, EPS_CLIP, ENTROPY_COEF, out=res).backward()

        by_torch()
        kernel()
        torch.cuda.synchronize()
        L = losses._ppo_loss_torch(probs, False, values, actions, old, returns, EPS_CLIP, ENTROPY_COEF)[0]
        worst = max(float((res.grad_dist - lp.grad).abs().max() / lp.grad.abs().max()), float((res.grad_values - lv.grad).abs().max() / lv.grad.abs().max()),
                    float((res.loss - L).abs() / L.abs()))
        if not worst <= 2.0 ** -40:
            raise SystemExit(f"n={n} A={na}: sgw_ppo_loss differs from the torch path by {worst:.3e} of the largest magnitude")
        wrapper()
        torch.cuda.synchronize()
        if not (torch.equal(kp.grad, res.grad_dist) and torch.equal(kv.grad, res.grad_values)):
            raise SystemExit(f"n={n} A={na}: ppo_loss(...).backward() differs from ppo_loss_terms")
        t_a, t_k, t_w, t_b = series((by_torch, kernel, wrapper, by_torch), args.reps, warm=3)
        (ma, la, ha), (mb, lb, hb), (mk, lk, hk), (mw, lw, hw) = stats(t_a), stats(t_b), stats(t_k), stats(t_w)
        base, spread = (ma + mb) / 2, abs(ma - mb)
        moved = n * (16 * na + 36)
        name = f"n={n} A={na}"
        emit(f"{name:22s} torch fwd+bwd {ma:10.1f} / {mb:10.1f} us (p10 {min(la, lb):.1f}, p90 {max(ha, hb):.1f}; spread of the medians {spread:.1f}); "
             f"outputs agree to {worst:.2e}")
        emit(f"{'':22s} sgw_ppo_loss  {mk:10.1f} us (p10 {lk:.1f}, p90 {hk:.1f})  x{base / mk:7.2f}  {'faster' if base - mk > spread else 'NOT faster'} than torch by more "
             f"than the spread; {moved / 1e6:.1f} MB algorithmic -> {moved / mk / 1e6:.3f} TB/s over the call's time (HBM peak 8 TB/s)")
        emit(f"{'':22s} ppo_loss().backward() {mw:10.1f} us (p10 {lw:.1f}, p90 {hw:.1f}): autograd's clone, multiplies and accumulation add {mw - mk:.1f} us")
        del probs, values, actions, old, returns, res, lp, lv, kp, kv, L
        torch.cuda.empty_cache()
    emit.close()


if __name__ == "__main__":
    main()
