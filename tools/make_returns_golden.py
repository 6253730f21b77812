"""TEST INFRASTRUCTURE ONLY -- generate ``tests/golden/returns/ppo_returns.npz`` from the reference's PPO learner.

Needs the reference checkout (``oracle/ref_loader.py``).  Usage::

    PYTHONDONTWRITEBYTECODE=1 python tools/make_returns_golden.py

What runs is the reference's own ``PyTorchPPO.train_step`` (``sorrel/models/pytorch/ppo.py``) with ``k_epochs=1`` on a hand-filled
``RolloutBuffer``, once per trajectory.  Nothing of it is restated: the raw float32 returns are read off the first list of length T the
call hands to ``torch.tensor`` (a wrapper around that function for the duration of the call), the normalised float64 tensor off the second
argument of ``model.loss_fn`` (a forward pre-hook).  Stored per trajectory ``i``: ``rewards_i`` / ``dones_i`` (float32), ``gamma_i``,
``returns_i`` (float32), ``normalized_i`` (float64); data only.

Rewards are integers in [-10, 10] times ``float32(0.37)``, symmetric about 0, so that products round.  The generator asserts what makes
the comparisons mean something: on the gamma 0.97 / 0.99 / 0.999 trajectories a single-rounding (fused multiply-add) restatement and a
float64 recurrence each differ from the reference somewhere; every column's std is > 0 (T >= 2); and the reference's normalised
values lie within a QUARTER of the tolerance the tests grant, ``8 T 2^-53 (1 + max|x| / (std + 1e-7))``, of the exactly rounded
result (rational arithmetic, 60-digit square root) -- so that bound is not what lets a wrong kernel pass."""
from __future__ import annotations

import decimal
import json
import os
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "returns", "ppo_returns.npz")
# (T, gamma, turns with done = 1, seed of the rewards)
TRAJECTORIES = (
    (1, 0.97, [0], 1),
    (2, 0.97, [], 2),
    (37, 0.97, [8, 20, 36], 3),
    (64, 0.99, [63], 4),
    (64, 0.5, [30], 5),
    (9, 0.0, [8], 6),
    (200, 0.999, [77, 199], 7),
)
ROUNDING_MATTERS = (0.97, 0.99, 0.999)


def reference_returns(ppo_module, torch, rewards, dones, gamma):
    """(raw float32 returns, normalised float64 returns) as one ``train_step`` of the reference computed them."""
    T = len(rewards)
    model = ppo_module.PyTorchPPO(input_size=(3,), action_space=2, layer_size=4, epsilon=0.0, device="cpu", entropy_coef=0.01,
                                  eps_clip=0.2, gamma=gamma, k_epochs=1, lr_actor=1e-3, lr_critic=1e-3, max_turns=T, seed=0)
    mem = model.memory
    rng = np.random.default_rng(T)
    mem.states[:] = rng.integers(0, 3, size=mem.states.shape)
    mem.actions[:] = rng.integers(0, 2, size=T)
    mem.log_probs[:] = np.log(0.5)
    mem.rewards[:] = rewards
    mem.dones[:] = dones
    mem.idx, mem.size = 0, T
    assert mem.rewards.dtype == np.float32 and mem.dones.dtype == np.float32
    seen = {}
    real_tensor = torch.tensor

    def tap(data, *args, **kwargs):
        if "raw" not in seen and isinstance(data, list) and len(data) == T:
            seen["raw"] = list(data)
        return real_tensor(data, *args, **kwargs)

    def pre(module, args):
        seen.setdefault("normalized", args[1].detach().clone())

    hook = model.loss_fn.register_forward_pre_hook(pre)
    torch.tensor = tap
    try:
        model.train_step()
    finally:
        torch.tensor = real_tensor
        hook.remove()
    raw = seen["raw"]
    assert all(isinstance(x, np.float32) for x in raw), "the reference's recurrence no longer runs in float32"
    normalized = seen["normalized"]
    assert normalized.dtype == torch.float64 and tuple(normalized.shape) == (T,)
    return np.asarray(raw, np.float32), normalized.numpy().copy()


def restated(rewards, dones, gamma, how):
    """NOT the reference: the two ways a device kernel could go wrong -- one rounding per step, or a float64 recurrence."""
    g32 = np.float32(gamma)
    out, d = np.zeros(len(rewards), np.float64), 0.0
    for t in range(len(rewards) - 1, -1, -1):
        if dones[t]:
            d = 0.0
        if how == "fma":
            d = float(np.float32(float(rewards[t]) + float(g32) * float(np.float32(d))))      # exact product, one rounding of the sum
        else:
            d = float(rewards[t]) + gamma * d
        out[t] = d
    return out


def exact_normalized(raw):
    """(x - mean) / (std + 1e-7) of the float32 values with the mean and the variance exact and the square root to 60 digits."""
    decimal.getcontext().prec = 60
    xs = [Fraction(float(x)) for x in raw]
    T = len(xs)
    mean = sum(xs) / T
    var = sum((x - mean) ** 2 for x in xs) / (T - 1)
    std = (decimal.Decimal(var.numerator) / decimal.Decimal(var.denominator)).sqrt()
    denom = std + decimal.Decimal("1e-7")
    out = [float((decimal.Decimal((x - mean).numerator) / decimal.Decimal((x - mean).denominator)) / denom) for x in xs]
    return np.asarray(out), float(std)


def main() -> None:
    ref_loader.install()
    import torch
    from sorrel.models.pytorch import ppo

    arrays, params = {}, []
    for i, (T, gamma, done_turns, seed) in enumerate(TRAJECTORIES):
        rng = np.random.default_rng(seed)
        half = rng.integers(-10, 11, size=(T + 1) // 2)
        ints = np.concatenate([half, -half])[:T]                    # symmetric about 0
        rng.shuffle(ints)
        rewards = (ints.astype(np.float32) * np.float32(0.37)).astype(np.float32)
        dones = np.zeros(T, np.float32)
        dones[done_turns] = 1.0
        raw, normalized = reference_returns(ppo, torch, rewards, dones, gamma)
        worst = 0.0
        if T == 1:
            assert np.isnan(normalized).all(), "one stored element normalises to NaN"
        else:
            exact, std = exact_normalized(raw)
            assert std > 0
            bound = 8 * T * 2.0 ** -53 * (1 + np.abs(raw.astype(np.float64)).max() / (std + 1e-7))
            worst = float(np.abs(normalized - exact).max() / bound)
            assert worst <= 0.25, f"trajectory {i}: the reference itself uses {worst:.3f} of the tolerance"
        if gamma in ROUNDING_MATTERS and T > 2:
            assert (restated(rewards, dones, gamma, "fma").astype(np.float32) != raw).any(), f"trajectory {i}: a fused multiply-add gives the same bits"
            assert (restated(rewards, dones, gamma, "f64") != raw.astype(np.float64)).any(), f"trajectory {i}: float64 gives the same values"
        arrays.update({f"rewards_{i}": rewards, f"dones_{i}": dones, f"gamma_{i}": np.float64(gamma), f"returns_{i}": raw,
                       f"normalized_{i}": normalized})
        params.append(dict(T=T, gamma=gamma, done_turns=done_turns, seed=seed, share_of_tolerance=worst))
        print(f"trajectory {i}: T={T} gamma={gamma} dones at {done_turns}; the reference uses {worst:.4f} of the tolerance")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, n=np.int64(len(TRAJECTORIES)), params=json.dumps(params), **arrays)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
