"""TEST INFRASTRUCTURE ONLY -- generate ``tests/golden/ppo_loss/clip_loss.npz`` from the reference's PPO learner.

Needs the reference checkout (``oracle/ref_loader.py``) and mpmath.  Usage::

    PYTHONDONTWRITEBYTECODE=1 python tools/make_ppo_loss_golden.py

What runs is the reference's own ``PyTorchPPO.train_step`` (``sorrel/models/pytorch/ppo.py``) with ``k_epochs=1`` on hand-filled
``RolloutBuffer``s, once per set.  Nothing of it is restated: forward hooks on ``policy.actor`` and ``policy.critic`` capture the two
networks' outputs and call ``retain_grad()`` on them, so that after the call's one ``backward`` their ``.grad`` is the gradient of
``loss.mean()`` at the actor's and at the critic's output; the normalised returns are the second argument of ``model.loss_fn`` (a forward
pre-hook, as ``tools/make_returns_golden.py`` taps them); ``policy.evaluate`` is wrapped for the duration of the call to keep its
log-probabilities and entropies.  Stored per set: probabilities, values, actions, old log-probabilities (float32, as the buffer holds
them) and returns; ``eps_clip`` and ``entropy_coef``; the mean loss the call returned; ``evaluate``'s log-probabilities and entropies;
the two gradients.  One set also stores the states, the reference's initial weights and every parameter's gradient (the end-to-end case
of ``tests/test_gpu_ppo_loss.py``).  Data only.

The stored ``log_probs`` of the buffer are hand-filled: the current policy's log-probability minus ``log`` of a chosen ratio, cycling over
ratios inside the clip range, above it and below it, so that with returns of both signs every gradient class occurs.  One set replaces the
actor by a module that returns hand-made UNNORMALISED rows with exact zeros and a probability of 1.

The generator asserts, on the CPU, what makes the comparisons mean something (``tests/ppo_loss_common.py`` holds the formulas):
every one of the five gradient classes occurs in every set with T >= 37; no ratio lies within a relative 2^-40 of ``lo`` or ``hi``;
outside the range the two surrogates differ by more than a relative 2^-40; apart from the hand-made rows no probability lies within
2^-40 of a clamp bound -- so another ``exp`` cannot change a branch --; and the reference's own results lie within a QUARTER of every
tolerance formula of an ``mpmath`` restatement (50 digits).  It prints the share the reference uses."""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_loader  # noqa: E402
from tests import ppo_loss_common as LC  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ppo_loss", "clip_loss.npz")
INPUTS, HIDDEN, GAMMA, ENTROPY_COEF = 6, 4, 0.97, 0.01
# (action_space, T, eps_clip); the last one is run a second time with the hand-made actor
SETS = ((2, 2, 0.2), (3, 37, 0.2), (4, 64, 0.2), (5, 200, 0.05), (9, 37, 0.05), (17, 64, 0.2), (2, 200, 0.05), (17, 200, 0.2), (4, 37, 0.05))
E2E = (4, 64, 0.2)
# ratios the stored log-probabilities are offset to, as multiples of eps_clip from 1: inside, above, below, ...
RATIO_STEPS = (0.0, 2.0, -2.0, 0.5, 3.0, -0.5, -3.0)


def states_of(T, na):
    r = np.arange(T)[:, None]
    c = np.arange(INPUTS)[None, :]
    return (((r * (2 * c + 3) + na * c * c + r * r // 7) % 17) - 8).astype(np.float64) * 0.75


def handmade_rows(T):
    base = np.array([[0.0, 0.5, 0.5, 0.0], [0.25, 0.0, 0.0, 0.75], [0.0, 0.0, 1.0, 0.0], [2.0, 0.0, 6.0, 0.0], [0.0, 0.0, 0.0, 1.0],
                     [0.0, 0.125, 0.0, 0.875], [3.0, 1.0, 2.0, 2.0], [0.0, 4.0, 0.0, 0.0], [0.5, 0.25, 0.125, 0.125], [1.0, 1.0, 1.0, 5.0]], np.float64)
    return base[np.arange(T) % len(base)]


def run_reference(ppo, torch, na, T, eps_clip, seed, handmade):
    model = ppo.PyTorchPPO(input_size=(INPUTS,), action_space=na, layer_size=HIDDEN, epsilon=0.0, device="cpu", entropy_coef=ENTROPY_COEF,
                           eps_clip=eps_clip, gamma=GAMMA, k_epochs=1, lr_actor=1e-3, lr_critic=1e-3, max_turns=T, seed=seed)
    torch.manual_seed(1000 + seed)
    model.policy = ppo.ActorCritic(INPUTS, na, HIDDEN)
    model.optimizer = torch.optim.Adam([{"params": model.policy.actor.parameters(), "lr": 1e-3}, {"params": model.policy.critic.parameters(), "lr": 1e-3}])
    with torch.no_grad():
        for net in (model.policy.actor, model.policy.critic):      # (the default initialisation leaves the outputs nearly constant: spread them)
            for layer in net:
                if isinstance(layer, torch.nn.Linear):
                    layer.weight.mul_(2.5)
    if handmade:
        class Rows(torch.nn.Module):
            def __init__(self, rows):
                super().__init__()
                self.rows = torch.nn.Parameter(torch.tensor(rows))

            def forward(self, states):
                return self.rows * 1.0

        model.policy.actor = Rows(handmade_rows(T))
    initial = {k: v.detach().clone().numpy() for k, v in model.policy.state_dict().items()}
    rng = np.random.default_rng(seed)
    states = states_of(T, na)
    actions = rng.integers(0, na, size=T)
    if handmade:                                                     # mostly actions that have weight; every fifth row whatever comes
        rows = handmade_rows(T)
        for k in range(T):
            if k % 5 and rows[k, actions[k]] == 0.0:
                actions[k] = int(np.argmax(rows[k]))
    half = rng.integers(-10, 11, size=(T + 1) // 2)
    ints = np.concatenate([half, -half])[:T]
    rng.shuffle(ints)
    rewards = (ints.astype(np.float32) * np.float32(0.37)).astype(np.float32)
    if T == 2:
        rewards = np.array([0.37, -1.11], np.float32)
    dones = np.zeros(T, np.float32)
    dones[T - 1] = 1.0
    if T > 40:
        dones[T // 3] = 1.0
    with torch.no_grad():
        lp_now, _v, _e = model.policy.evaluate(torch.tensor(states), torch.tensor(actions, dtype=torch.float64))
    steps = np.array([RATIO_STEPS[(k + k // 7) % len(RATIO_STEPS)] for k in range(T)])
    old = (lp_now.numpy() - np.log(1.0 + steps * eps_clip)).astype(np.float32)
    mem = model.memory
    mem.states[:] = states
    mem.actions[:] = actions
    mem.log_probs[:] = old
    mem.rewards[:] = rewards
    mem.dones[:] = dones
    mem.idx, mem.size = 0, T
    assert mem.log_probs.dtype == np.float32
    seen = {}

    def keep(name):
        def hook(module, args, output):
            output.retain_grad()
            seen[name] = output
        return hook

    def pre(module, args):
        seen.setdefault("returns", args[1].detach().clone())

    real_evaluate = model.policy.evaluate

    def evaluate(state, action):
        out = real_evaluate(state, action)
        seen["log_probs"], seen["entropies"] = out[0].detach().clone(), out[2].detach().clone()
        return out

    hooks = [model.policy.actor.register_forward_hook(keep("probs")), model.policy.critic.register_forward_hook(keep("values")),
             model.loss_fn.register_forward_pre_hook(pre)]
    model.policy.evaluate = evaluate
    try:
        loss = model.train_step()
    finally:
        del model.policy.evaluate
        for h in hooks:
            h.remove()
    probs, values = seen["probs"], seen["values"]
    assert probs.dtype == torch.float64 and tuple(probs.shape) == (T, na) and tuple(values.shape) == (T, 1)
    grads = {k: p.grad.detach().clone().numpy() for k, p in model.policy.named_parameters()}
    return dict(probs=probs.detach().numpy().copy(), values=values.detach().numpy().reshape(T).copy(), actions=actions.astype(np.int64),
                old_log_probs=old, returns=seen["returns"].numpy().copy(), loss=np.float64(loss), log_probs=seen["log_probs"].numpy().copy(),
                entropies=seen["entropies"].numpy().copy(), grad_probs=probs.grad.numpy().copy(), grad_values=values.grad.numpy().reshape(T).copy(),
                states=states, initial=initial, param_grads=grads)


def exact(s, eps_clip, c, vc=0.5):
    """The contract's mathematics (not its order) at 50 digits from the stored inputs: lp, H, gradients and L, as floats."""
    import mpmath as mp

    mp.mp.dps = 50
    x, n, na = s["probs"], s["probs"].shape[0], s["probs"].shape[1]
    lo_c, hi_c = mp.mpf(2) ** -52, 1 - mp.mpf(2) ** -52
    lo, hi = mp.mpf(1.0 - eps_clip), mp.mpf(1.0 + eps_clip)
    c, vc = mp.mpf(c), mp.mpf(vc)
    lps, Hs, gd, gv, tot = [], [], np.zeros((n, na)), np.zeros(n), mp.mpf(0)
    for k in range(n):
        w = [mp.mpf(float(e)) for e in x[k]]
        S = mp.fsum(w)
        q = [e / S for e in w]
        l = [mp.log(min(max(e, lo_c), hi_c)) for e in q]
        u = [lo_c <= e <= hi_c for e in q]
        a = int(s["actions"][k])
        H = -mp.fsum(qi * li for qi, li in zip(q, l))
        v, R, old = mp.mpf(float(s["values"][k])), mp.mpf(float(s["returns"][k])), mp.mpf(float(s["old_log_probs"][k]))
        r = mp.exp(l[a] - old)
        A = R - v
        s1, s2 = r * A, min(max(r, lo), hi) * A
        inside = lo <= r <= hi
        gr = A if s1 < s2 else ((A if inside else 0) if s1 > s2 else A / 2 + (A / 2 if inside else 0))
        gl = [c * qi for qi in q]
        gl[a] -= gr * r
        gq = [(gl[i] / q[i] if u[i] else 0) + c * l[i] for i in range(na)]
        t = mp.fsum(gq[i] * q[i] for i in range(na))
        for j in range(na):
            gd[k, j] = float((gq[j] - t) / S / n)
        gv[k] = float(2 * vc * (v - R) / n)
        tot += -min(s1, s2) - c * H
        lps.append(float(l[a]))
        Hs.append(float(H))
    M = mp.fsum((mp.mpf(float(v)) - mp.mpf(float(R))) ** 2 for v, R in zip(s["values"], s["returns"])) / n
    return dict(lp=np.array(lps), H=np.array(Hs), grad_dist=gd, grad_values=gv, L=float(tot / n + vc * M))


def main() -> None:
    ref_loader.install()
    import torch
    from sorrel.models.pytorch import ppo

    arrays, meta = {}, dict(sets=[])
    runs = [(na, T, eps, False) for na, T, eps in SETS] + [(4, 40, 0.2, True)]
    for i, (na, T, eps, handmade) in enumerate(runs):
        tag = f"{'hand' if handmade else na}_{T}_{str(eps).replace('.', 'p')}"
        s = run_reference(ppo, torch, na, T, eps, 10 + i, handmade)
        info = LC.restate(s["probs"], False, s["values"], s["actions"], s["old_log_probs"], s["returns"], eps, ENTROPY_COEF)
        assert not info["bad"].any()
        cls, mar = LC.classes(info), LC.branch_margins(info)
        if T >= 37:
            assert all(v > 0 for v in cls.values()), f"{tag}: a gradient class does not occur: {cls}"
        assert mar["ratio"] > LC.MARGIN, f"{tag}: a ratio lies {mar['ratio']:.3e} from a clip bound"
        assert mar["surrogates"] > LC.MARGIN, f"{tag}: surrogates {mar['surrogates']:.3e} apart outside the range"
        if not handmade:
            assert mar["clamp_rows"].min() > LC.MARGIN, f"{tag}: a probability lies at a clamp bound"
        tol, ex = LC.tolerances(info), exact(s, eps, ENTROPY_COEF)
        share = dict(lp=np.abs(s["log_probs"] - ex["lp"]) / tol["lp"], H=np.abs(s["entropies"] - ex["H"]) / tol["H"],
                     grad_dist=np.abs(s["grad_probs"] - ex["grad_dist"]) / tol["grad_dist"],
                     grad_values=np.abs(s["grad_values"] - ex["grad_values"]) / np.maximum(tol["grad_values"], 1e-300),
                     L=np.abs(s["loss"] - ex["L"]) / tol["L"])
        share = {k: float(np.nanmax(v)) for k, v in share.items()}
        ours = dict(lp=np.abs(info["lp"] - ex["lp"]) / tol["lp"], H=np.abs(info["H"] - ex["H"]) / tol["H"],
                    grad_dist=np.abs(info["grad_dist"] - ex["grad_dist"]) / tol["grad_dist"],
                    grad_values=np.abs(info["grad_values"] - ex["grad_values"]) / np.maximum(tol["grad_values"], 1e-300), L=np.abs(info["L"] - ex["L"]) / tol["L"])
        ours = {k: float(np.nanmax(v)) for k, v in ours.items()}
        assert max(share.values()) <= 0.25, f"{tag}: the reference itself uses {share} of the tolerances"
        assert max(ours.values()) <= 0.25, f"{tag}: the restatement uses {ours} of the tolerances"
        print(f"{tag}: classes {cls}; margins ratio {mar['ratio']:.2e} surrogates {mar['surrogates']:.2e}; share of the tolerance the reference uses "
              + " ".join(f"{k} {v:.4f}" for k, v in share.items()) + "; the restatement " + " ".join(f"{k} {v:.4f}" for k, v in ours.items()))
        for k in ("probs", "values", "actions", "old_log_probs", "returns", "log_probs", "entropies", "grad_probs", "grad_values", "loss"):
            arrays[f"{k}_{tag}"] = s[k]
        meta["sets"].append(dict(tag=tag, na=na, T=T, eps_clip=eps, entropy_coef=ENTROPY_COEF, exact=handmade, classes=cls, share=share))
        if (na, T, eps) == E2E and not handmade:
            names = sorted(s["initial"])
            meta["e2e"] = dict(tag=tag, inputs=INPUTS, hidden=HIDDEN, names=names)
            arrays["e2e_states"] = s["states"]
            for name in names:
                arrays["e2e_w:" + name] = s["initial"][name]
                arrays["e2e_g:" + name] = s["param_grads"][name]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, params=json.dumps(meta), **arrays)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
