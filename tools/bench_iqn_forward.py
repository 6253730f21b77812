#!/usr/bin/env python3
"""IQN's network forward on the device: ``sgw_iqn_forward`` (``IQN.quantiles(out=)``, two launches) against the torch path it replaces
(``IQN.forward`` under ``no_grad``: the reference's sequence of ops).  Prints the text of profiles/iqn_forward.txt.

usage: python tools/bench_iqn_forward.py [--reps 20] [--out FILE] [--no-cos]

First the one thing the tests cannot restate: the device library's ``cosf``.  ``out_cos`` of 2^20 uniform taus x 64 frequencies (16 384
rows of 64 quantiles through a one-unit network) against float64 ``cos`` of the same float32 argument, the maximum in units of 2^-24.
The GPU test asserts twice that figure, rounded up to a whole unit.

Then the timing.  Shapes: 1 024 / 16 384 / 65 536 rows of the reference's network (875 inputs, layer size 250, 12 quantiles, 4 actions),
and the same rows of a smaller one (layer size 64, 8 quantiles).  Both paths are timed in one process with device events around every
call and alternate call by call after a warm-up: torch, kernel, torch again.  The torch path is the baseline and is therefore timed
TWICE per round: the difference between the medians of its two series is the spread a difference between paths has to exceed.  Before
any timing the outputs are compared on the timed data with the same taus (the tests hold the bound as a formula; here the quantiles must
agree to 1e-4 of the largest magnitude and the greedy actions are counted).  FLOP: ``2 n (D L + N (64 L + L L + L (A + 1)))``; the
achieved rate is set against the chip's 155 TFLOP/s of float32-input matrix instructions."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import torch  # noqa: E402
from _timing import Emitter, series, stats  # noqa: E402  (tools/_timing.py)

from sorrel_amd.models import iqn as M  # noqa: E402

PEAK_TF = 155.0
SHAPES = tuple((n, 875, 250, 12, 4) for n in (1024, 16384, 65536)) + tuple((n, 875, 64, 8, 4) for n in (1024, 16384, 65536))


def cos_sweep(dev, emit):
    net = M.IQN((1,), 1, 1, seed=1, n_quantiles=64, n_frames=1, device=dev).eval()
    worst = 0.0
    n = 16384
    gen = torch.Generator(device=dev).manual_seed(7)
    taus = torch.rand((n, 64), device=dev, generator=gen)
    taus[0, 0], taus[0, 1] = 0.0, 1.0 - 2.0 ** -24                                  # the ends of the range
    res = net.quantiles(torch.zeros((n, 1), device=dev), taus=taus, cos=True)
    args = (taus.reshape(n, 64, 1) * net.pis).double()
    err = (res.cos.double() - torch.cos(args)).abs() * 2.0 ** 24
    worst = float(err.max())
    at = int(err.argmax())
    emit(f"cosf: out_cos of {n * 64} uniform taus x 64 frequencies (arguments in [0, 64 pi)) against float64 cos of the same float32 argument: "
         f"at most {worst:.4f} x 2^-24 (at argument {float(args.reshape(-1)[at]):.6f}); mean {float(err.mean()):.4f}")
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-cos", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_iqn_forward needs a HIP device")
    emit = Emitter(args.out)

    dev = torch.device("cuda:0")
    emit(f"# tools/bench_iqn_forward.py --reps {args.reps}: {torch.cuda.get_device_name(0)}; float32 states and weights, eval mode; microseconds per call, "
         f"device events around each call, paths alternating call by call (torch, kernel, torch)")
    if not args.no_cos:
        cos_sweep(dev, emit)
    torch.manual_seed(3)
    for n, D, L, Nq, A in SHAPES:
        net = M.IQN((D,), A, L, seed=5, n_quantiles=Nq, n_frames=1, device=dev).eval()
        x = torch.randn((n, D), device=dev)
        taus = torch.rand((n, Nq), device=dev)
        res = M.IQNOutput(n, Nq, A, L, dev)

        def by_torch():
            with torch.no_grad():
                return net(x, Nq)

        def kernel():
            net.quantiles(x, taus=taus, out=res)

        kernel()
        torch.cuda.synchronize()
        # the same taus through the torch ops
        net.calc_cos = lambda b, k: (torch.cos(taus.reshape(b, k, 1) * net.pis), taus.reshape(b, k, 1))
        quant, _ = by_torch()
        del net.calc_cos
        scale = float(quant.abs().max())
        worst = float((quant - res.quantiles).abs().max()) / scale
        same = float((quant.mean(dim=1).argmax(dim=1) == res.qvalues.argmax(dim=1)).float().mean())
        del quant
        if not worst <= 1e-4:
            raise SystemExit(f"n={n} L={L} N={Nq}: sgw_iqn_forward differs from the torch path by {worst:.3e} of the largest magnitude")
        t_a, t_k, t_b = series((by_torch, kernel, by_torch), args.reps, warm=3)
        (ma, la, ha), (mb, lb, hb), (mk, lk, hk) = stats(t_a), stats(t_b), stats(t_k)
        base, spread = (ma + mb) / 2, abs(ma - mb)
        flop = 2.0 * n * (D * L + Nq * (64 * L + L * L + L * (A + 1)))
        name = f"n={n} D={D} L={L} N={Nq} A={A}"
        emit(f"{name:32s} torch no_grad   {ma:10.1f} / {mb:10.1f} us (p10 {min(la, lb):.1f}, p90 {max(ha, hb):.1f}; spread of the medians {spread:.1f}); "
             f"quantiles agree to {worst:.2e} of the largest, greedy actions equal in {same:.4f} of the rows")
        emit(f"{'':32s} sgw_iqn_forward {mk:10.1f} us (p10 {lk:.1f}, p90 {hk:.1f})  x{base / mk:7.2f}  "
             f"{'faster' if base - mk > spread else ('SLOWER' if mk - base > spread else 'the same within the spread')} than torch; {flop / 1e9:.2f} GFLOP -> "
             f"{flop / mk / 1e6:.2f} TFLOP/s over the call's time ({100 * flop / mk / 1e6 / PEAK_TF:.1f} % of {PEAK_TF:.0f}); torch {flop / base / 1e6:.2f} TFLOP/s")
        del net, x, taus, res
        torch.cuda.empty_cache()
    emit.close()


if __name__ == "__main__":
    main()
