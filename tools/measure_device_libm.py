#!/usr/bin/env python3
"""How far the device's float64 ``log`` and ``exp`` lie from the exact value over the arguments the PPO-loss fixture produces
(``tests/golden/ppo_loss/clip_loss.npz``): the figure ``tests/ppo_loss_common.py`` doubles into ``LIBM_ULPS``.  Needs
a HIP device and mpmath.

usage: python tools/measure_device_libm.py [--out FILE]

Arguments: for ``log`` every clamped probability ``q_i`` of every fixture row; for ``exp`` every ``lp - old`` and, as a logits model would
hand them over, every ``log q_i - max_j log q_j``.  The device values are torch's elementwise float64 ``log`` / ``exp``, which call the
same ROCm device-library routines a HIP kernel's ``log(double)`` / ``exp(double)`` resolve to; for ``exp`` the kernel's own use is measured
as well: one-action rows (``lp = -2^-52``), ``A = -1`` and a clip range wide open make the row's policy term ``P = exp(lp - old)``, read from
``out_row_terms``.  The exact values are mpmath's at 50 digits; the error is in units of ``2^-52`` of the exact value's magnitude (at
most one unit in the last place).  The host's NumPy is measured beside it."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mpmath as mp  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import ppo_loss_common as LC  # noqa: E402


def error_in_units(got, args, fn):
    mp.mp.dps = 50
    worst = 0.0
    for g, a in zip(got.tolist(), args.tolist()):
        exact = fn(mp.mpf(a))
        if exact == 0:
            continue
        worst = max(worst, float(abs(mp.mpf(g) - exact) / abs(exact) * mp.mpf(2) ** 52))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_device_libm needs a HIP device")
    from sorrel_amd import losses

    sets, _ = LC.load_fixture()
    log_args, exp_args = [], []
    for s in sets.values():
        info = LC.restate(s["probs"], False, s["values"], s["actions"], s["old_log_probs"], s["returns"], s["eps_clip"], s["entropy_coef"])
        q = np.clip(info["q"], LC.EPS_LO, LC.EPS_HI)
        log_args.append(q.ravel())
        exp_args.append(info["lp"] - s["old_log_probs"].astype(np.float64))
        lg = np.log(q)
        exp_args.append((lg - lg.max(axis=1, keepdims=True)).ravel())
    log_args, exp_args = np.unique(np.concatenate(log_args)), np.unique(np.concatenate(exp_args))
    lines = [f"# tools/measure_device_libm.py: {torch.cuda.get_device_name(0)}; errors in units of 2^-52 of the exact value (mpmath, 50 digits)"]
    dev = "cuda:0"
    d_log = torch.log(torch.from_numpy(log_args).to(dev)).cpu().numpy()
    d_exp = torch.exp(torch.from_numpy(exp_args).to(dev)).cpu().numpy()
    lines.append(f"log over {len(log_args)} arguments in [{log_args.min():.3e}, {log_args.max():.6f}]: device {error_in_units(d_log, log_args, mp.log):.4f}, "
                 f"host NumPy {error_in_units(np.log(log_args), log_args, mp.log):.4f}")
    lines.append(f"exp over {len(exp_args)} arguments in [{exp_args.min():.4f}, {exp_args.max():.4f}]: device {error_in_units(d_exp, exp_args, mp.exp):.4f}, "
                 f"host NumPy {error_in_units(np.exp(exp_args), exp_args, mp.exp):.4f}")
    # the kernel's own exp: P = exp(lp - old) with lp = -2^-52 (one action), A = -1, the clip range wide open
    old = np.unique(exp_args.astype(np.float32))
    n = len(old)
    res = losses.ppo_loss_terms(torch.ones((n, 1), dtype=torch.float64, device=dev), torch.ones(n, dtype=torch.float64, device=dev),
                                torch.zeros(n, dtype=torch.int64, device=dev), torch.from_numpy(-old).to(dev), torch.zeros(n, dtype=torch.float64, device=dev),
                                1e300, 0.0, row_terms=True)
    k_args = -2.0 ** -52 + old.astype(np.float64)                          # (the subtraction the kernel performs, rounded as it rounds)
    k_exp = res.row_terms[:, 0].cpu().numpy()
    lines.append(f"exp inside sgw_ppo_loss over {n} float32 arguments: {error_in_units(k_exp, k_args, mp.exp):.4f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
