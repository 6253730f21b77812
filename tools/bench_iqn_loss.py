#!/usr/bin/env python3
"""IQN's quantile Huber loss on the device: ``sgw_iqn_loss`` against the torch path it replaces (``sorrel_amd.losses._iqn_loss_torch``:
the reference's lines as torch ops, forward AND backward through autograd).  Prints the text of profiles/iqn_loss.txt.

usage: python tools/bench_iqn_loss.py [--reps 20] [--out FILE]

Shapes: batches of 64 (the reference's), 1 024 and 65 536 rows, crossed with 12 (the reference's default) and 32 quantiles, crossed with
4 / 8 / 16 actions; float32 quantile tensors, int64 actions, float64 ``valid`` (what the reference's ``Buffer.sample`` returns), a
quarter of the rows done and a fifth invalid.  One action of every row of ``q_next_local`` is lifted clear of the others, so that the
order in which torch's ``mean`` adds cannot move an argmax and the two paths compare row for row.

Both paths are timed in one process with device events around every call and alternate call by call after a warm-up: torch, kernel,
torch again.  The torch path is the baseline and is therefore timed TWICE per round: the difference between the medians of its two
series is the spread a difference between paths has to exceed.  ``kernel`` is ``iqn_loss_terms(out=)`` (two launches, nothing
allocated).  Before any timing the outputs are compared on the timed data (the tests hold the tolerance formulas; here the chosen
actions must be equal, the gradient within ``N 2^-23`` of its largest magnitude and the loss within 2^-40 relative).  Algorithmic
bytes: ``16 B N A`` -- three float32 ``[B, N, A]`` tensors read and one written."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import torch  # noqa: E402
from _timing import Emitter, series, stats  # noqa: E402  (tools/_timing.py)

from sorrel_amd import losses  # noqa: E402

DISCOUNT = 0.99 ** 3
SHAPES = tuple((B, N, A) for B in (64, 1024, 65536) for N in (12, 32) for A in (4, 8, 16))


def batch(B, N, A, dev):
    qe, ql, qt = (torch.randn((B, N, A), device=dev) * 1.5 for _ in range(3))
    ql.scatter_add_(2, torch.randint(0, A, (B, 1, 1), device=dev).expand(B, N, 1), torch.full((B, N, 1), 12.0, device=dev))
    taus = torch.rand((B, N, 1), device=dev)
    actions = torch.randint(0, A, (B, 1), device=dev)
    rewards = torch.randn((B, 1), device=dev)
    dones = (torch.rand((B, 1), device=dev) < 0.25).float()
    valid = (torch.rand((B, 1), device=dev) >= 0.2).double()
    return qe, taus, ql, qt, actions, rewards, dones, valid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_iqn_loss needs a HIP device")
    emit = Emitter(args.out)

    dev = torch.device("cuda:0")
    emit(f"# tools/bench_iqn_loss.py --reps {args.reps}: {torch.cuda.get_device_name(0)}; discount {DISCOUNT:.6f}; float32 quantiles, float64 valid; "
         f"microseconds per call, device events around each call, paths alternating call by call (torch, kernel, torch)")
    torch.manual_seed(3)
    for B, N, A in SHAPES:
        qe, taus, ql, qt, actions, rewards, dones, valid = batch(B, N, A, dev)
        res = losses.iqn_loss_terms(qe, taus, ql, qt, actions, rewards, dones, valid, DISCOUNT)
        leaf = qe.clone().requires_grad_(True)

        def by_torch():
            leaf.grad = None
            losses._iqn_loss_torch(leaf, taus, ql, qt, actions, rewards, dones, valid, DISCOUNT)[0].backward()

        def kernel():
            losses.iqn_loss_terms(qe, taus, ql, qt, actions, rewards, dones, valid, DISCOUNT, out=res)

        by_torch()
        kernel()
        torch.cuda.synchronize()
        L, _td, a_star, _ql = losses._iqn_loss_torch(qe, taus, ql, qt, actions, rewards, dones, valid, DISCOUNT)
        if not torch.equal(a_star, res.next_actions):
            raise SystemExit(f"B={B} N={N} A={A}: the chosen actions differ in {int((a_star != res.next_actions).sum())} rows")
        worst_g = float((res.grad_expected - leaf.grad).abs().max() / leaf.grad.abs().max())
        worst_l = float((res.loss - L).abs() / L.abs())
        if not (worst_g <= N * 2.0 ** -23 and worst_l <= 2.0 ** -40):
            raise SystemExit(f"B={B} N={N} A={A}: sgw_iqn_loss differs from the torch path: gradient {worst_g:.3e} of the largest magnitude, loss {worst_l:.3e}")
        t_a, t_k, t_b = series((by_torch, kernel, by_torch), args.reps, warm=3)
        (ma, la, ha), (mb, lb, hb), (mk, lk, hk) = stats(t_a), stats(t_b), stats(t_k)
        base, spread = (ma + mb) / 2, abs(ma - mb)
        moved = 16 * B * N * A
        name = f"B={B} N={N} A={A}"
        emit(f"{name:20s} torch fwd+bwd {ma:10.1f} / {mb:10.1f} us (p10 {min(la, lb):.1f}, p90 {max(ha, hb):.1f}; spread of the medians {spread:.1f}); "
             f"gradient agrees to {worst_g:.2e}, loss to {worst_l:.2e}")
        emit(f"{'':20s} sgw_iqn_loss  {mk:10.1f} us (p10 {lk:.1f}, p90 {hk:.1f})  x{base / mk:7.2f}  {'faster' if base - mk > spread else 'NOT faster'} than torch by more "
             f"than the spread; {moved / 1e6:.3f} MB algorithmic -> {moved / mk / 1e6:.4f} TB/s over the call's time (HBM peak 8 TB/s)")
        del qe, taus, ql, qt, actions, rewards, dones, valid, res, leaf, L, _td, a_star, _ql
        torch.cuda.empty_cache()
    emit.close()


if __name__ == "__main__":
    main()
