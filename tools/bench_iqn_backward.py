#!/usr/bin/env python3
"""IQN's forward + backward on the device: ``IQN.forward_fused`` + ``backward()`` (``sgw_iqn_forward``, then one ``sgw_iqn_backward`` call)
against the path it replaces, ``IQN.forward`` + torch's autograd ``backward()``.  Prints the text of profiles/iqn_backward.txt.

usage: python tools/bench_iqn_backward.py [--reps 20] [--out FILE]

The reference's shape (in_features 875, layer_size 250, 12 quantiles, 4 actions), training mode, batches of 64 (the reference's), 1 024
and 4 096 states; float32 states; the incoming gradient is a fixed random ``[B, N, A]`` tensor, so a timed call is
``q, _ = net(...); q.backward(g)`` with the parameters' ``.grad`` set to None before it (untimed).

Both paths are timed in one process with device events around every call and alternate call by call after a warm-up: torch, kernel,
torch again.  The torch path is the baseline and is therefore timed TWICE per round: the difference between the medians of its two
series is the spread a difference between paths has to exceed.  Before any timing the gradients of the two paths are compared on the timed
data with the same taus and the same noise (the tests hold the cap; here the largest difference per tensor relative to the tensor's
largest magnitude is printed).  The weight gradients of ``sgw_iqn_backward`` are serial in the batch rows: nothing is asserted about
speed; the numbers are reported as they come."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import torch  # noqa: E402
from _timing import Emitter, series, stats  # noqa: E402  (tools/_timing.py)

from sorrel_amd.models.iqn import IQN  # noqa: E402

D, L, NQ, A = 875, 250, 12, 4
BATCHES = (64, 1024, 4096)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_iqn_backward needs a HIP device")
    emit = Emitter(args.out, as_it_grows=True)
    dev = torch.device("cuda:0")
    emit(f"# tools/bench_iqn_backward.py --reps {args.reps}: {torch.cuda.get_device_name(0)}; in_features {D}, layer_size {L}, {NQ} quantiles, "
         f"{A} actions, training mode; microseconds per forward + backward, device events around each call, paths alternating call by call "
         f"(torch, kernel, torch)")
    torch.manual_seed(5)
    net = IQN((D,), A, L, seed=5, n_quantiles=NQ, n_frames=1).to(dev).train(True)
    params = list(net.parameters())
    for B in BATCHES:
        x = torch.randn((B, D), device=dev)
        g = torch.randn((B, NQ, A), device=dev)
        taus = torch.rand((B, NQ), device=dev)

        def clear():
            for p in params:
                p.grad = None

        def by_torch():
            clear()
            q, _ = net(x, NQ)
            q.backward(g)

        def by_kernel():
            clear()
            q, _ = net.forward_fused(x, taus=taus)
            q.backward(g)

        # the two paths on the same taus and the same noise: how far apart are their gradients?
        real_normal, real_rand = torch.Tensor.normal_, torch.rand
        torch.Tensor.normal_ = lambda t, *a, **k: t
        torch.rand = lambda *shape, **kw: taus.cpu().reshape(shape)
        try:
            by_torch()
            ref = [p.grad.clone() for p in params]
            by_kernel()
            far = max(float((p.grad - r).abs().max() / r.abs().max().clamp_min(1e-30)) for p, r in zip(params, ref))
        finally:
            torch.Tensor.normal_, torch.rand = real_normal, real_rand
        t1, tk, t2 = series((by_torch, by_kernel, by_torch), args.reps, 3)
        (m1, lo1, hi1), (mk, lok, hik), (m2, _, _) = stats(t1), stats(tk), stats(t2)
        spread = abs(m1 - m2)
        base = 0.5 * (m1 + m2)
        verdict = ("faster than torch by more than the spread" if mk < base - spread else
                   "SLOWER than torch by more than the spread" if mk > base + spread else "within the spread of torch")
        emit(f"B={B:<5} n N={B * NQ:<6} torch fwd+bwd     {m1:9.1f} / {m2:9.1f} us (p10 {lo1:.1f}, p90 {hi1:.1f}; spread of the medians {spread:.1f}); "
             f"gradients agree to {far:.2e} of a tensor's largest")
        emit(f"{'':21}forward_fused+bwd {mk:9.1f} us (p10 {lok:.1f}, p90 {hik:.1f})  x {base / mk:6.2f}  {verdict}")
    emit.close()


if __name__ == "__main__":
    main()
