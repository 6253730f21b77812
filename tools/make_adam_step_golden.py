"""TEST INFRASTRUCTURE ONLY -- generate ``tests/golden/adam_step/{iqn,ppo}.npz`` from the reference's own learners.

Needs the reference checkout (``oracle/ref_loader.py``).  Usage::

    PYTHONDONTWRITEBYTECODE=1 python tools/make_adam_step_golden.py

What runs is the reference's own ``iRainbowModel.train_step`` (a small model: ``layer_size=8``, ``n_frames=2``, 4 actions, 4 quantiles,
a hand-filled ``Buffer``; four steps) and ``PyTorchPPO.train_step`` (``lr_actor != lr_critic``, ``k_epochs=3``, float64) on the CPU.
Nothing of them is restated: ``clip_grad_norm_`` is wrapped in the IQN module's namespace, ``optimizer.step`` and ``soft_update`` on the
instances, and the wrappers record per step the gradients before and after clipping, the returned norm, the parameters and Adam's
state before and after, and the targets before and after.  Data only.

The rewards and the states are scaled between the IQN steps so that the norm lies above ``max_norm`` in some steps and below it in others; the
generator asserts both.  It also measures how much of each tolerance formula of ``tests/adam_step_common.py`` the reference's own results
use against the restatement fed with the reference's coefficient, prints the shares and asserts at most a half; ``exp_avg``,
``exp_avg_sq`` and the targets must match bit for bit (``meta['moments_exact']`` records whether they did)."""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_loader  # noqa: E402
from tests import adam_step_common as AC  # noqa: E402

OBS, N_FRAMES, ACTIONS, QUANTILES, BATCH = 3, 2, 4, 4, 16
# per IQN step, (rewards, states): two norms above 1, two below (Huber bounds dL/dq whatever the rewards are, so the states are scaled too)
SCALES = ((40.0, 30.0), (0.002, 1.0), (25.0, 30.0), (0.001, 1.0))
PER_TENSOR_IQN = ("grad", "grad_clipped", "param_before", "param_after", "exp_avg_before", "exp_avg_after", "exp_avg_sq_before",
                  "exp_avg_sq_after", "target_before", "target_after")
PER_TENSOR_PPO = tuple(k for k in PER_TENSOR_IQN if not k.startswith(("target", "grad_clipped")))


def arrays_of(tensors):
    return [t.detach().clone().numpy() for t in tensors]


def wrap_optimizer(optimizer, params, steps, torch):
    real = optimizer.step

    def step(*a, **k):
        rec = steps[-1] if steps and "param_after" not in steps[-1] else {}
        if not rec:
            steps.append(rec)
        assert all(p.grad is not None for p in params)
        rec.setdefault("grad", arrays_of(p.grad for p in params))
        rec["param_before"] = arrays_of(params)
        for key in ("exp_avg", "exp_avg_sq"):
            rec[key + "_before"] = [optimizer.state[p][key].clone().numpy() if p in optimizer.state and key in optimizer.state[p]
                                    else np.zeros(tuple(p.shape), p.detach().numpy().dtype) for p in params]
        out = real(*a, **k)
        rec["param_after"] = arrays_of(params)
        for key in ("exp_avg", "exp_avg_sq"):
            rec[key + "_after"] = [optimizer.state[p][key].clone().numpy() for p in params]
        rec["step"] = np.int64(int(optimizer.state[params[0]]["step"]))
        assert all(int(optimizer.state[p]["step"]) == int(rec["step"]) for p in params)
        return out

    optimizer.step = step


def run_iqn(torch):
    from sorrel.models.pytorch import iqn

    cap = BATCH + N_FRAMES + 6
    model = iqn.iRainbowModel(input_size=(OBS,), action_space=ACTIONS, layer_size=8, epsilon=0.0, device="cpu", seed=5, n_frames=N_FRAMES,
                              n_step=3, batch_size=BATCH, memory_size=cap, n_quantiles=QUANTILES, TAU=0.01)
    rng = np.random.default_rng(11)
    mem = model.memory
    base_states = rng.normal(size=mem.states.shape).astype(np.float32)
    mem.actions[:] = rng.integers(0, ACTIONS, size=cap)
    base_rewards = rng.integers(-4, 5, size=cap).astype(np.float32)
    mem.dones[:] = (rng.random(size=cap) < 0.2).astype(np.float32)
    mem.idx, mem.size = 0, cap
    params, targets = list(model.qnetwork_local.parameters()), list(model.qnetwork_target.parameters())
    with torch.no_grad():                      # (both nets start from one seed: move the target off the local net)
        for t in targets:
            t.add_(torch.from_numpy(rng.normal(0.0, 0.05, size=tuple(t.shape)).astype(np.float32)))
    steps = []
    real_clip, real_soft = iqn.clip_grad_norm_, model.soft_update

    def clip(parameters, max_norm, *a, **k):
        ps = list(parameters)
        assert len(ps) == len(params) and all(x is y for x, y in zip(ps, params)) and not a and not k
        rec = dict(grad=arrays_of(p.grad for p in ps))
        norm = real_clip(ps, max_norm)
        rec["grad_clipped"], rec["norm"], rec["max_norm"] = arrays_of(p.grad for p in ps), norm.detach().numpy().copy(), np.float64(max_norm)
        steps.append(rec)
        return norm

    def soft_update():
        steps[-1]["target_before"] = arrays_of(targets)
        real_soft()
        steps[-1]["target_after"] = arrays_of(targets)

    wrap_optimizer(model.optimizer, params, steps, torch)
    iqn.clip_grad_norm_, model.soft_update = clip, soft_update
    np.random.seed(3)
    torch.manual_seed(3)
    try:
        for reward_scale, state_scale in SCALES:
            mem.rewards[:] = base_rewards * np.float32(reward_scale)
            mem.states[:] = base_states * np.float32(state_scale)
            model.train_step()
    finally:
        iqn.clip_grad_norm_ = real_clip
    group = model.optimizer.param_groups[0]
    meta = dict(dtype="float32", tensors=len(params), steps=len(steps), lrs=[group["lr"]] * len(params), betas=list(group["betas"]),
                eps=group["eps"], tau=model.TAU, max_norm=1.0, per_tensor=list(PER_TENSOR_IQN), per_step=["norm", "step"],
                shapes=[list(p.shape) for p in params])
    return meta, steps


def run_ppo(torch):
    from sorrel.models.pytorch import ppo

    T, inputs, na = 24, 5, 3
    model = ppo.PyTorchPPO(input_size=(inputs,), action_space=na, layer_size=6, epsilon=0.0, device="cpu", entropy_coef=0.01, eps_clip=0.2,
                           gamma=0.95, k_epochs=3, lr_actor=3e-4, lr_critic=1e-3, max_turns=T, seed=7)
    rng = np.random.default_rng(13)
    states = rng.normal(size=(T, inputs))
    actions = rng.integers(0, na, size=T)
    with torch.no_grad():
        lp, _v, _e = model.policy.evaluate(torch.tensor(states), torch.tensor(actions, dtype=torch.float64))
    mem = model.memory
    mem.states[:] = states
    mem.actions[:] = actions
    mem.log_probs[:] = (lp.numpy() - rng.normal(0.0, 0.1, size=T)).astype(np.float32)
    mem.rewards[:] = rng.integers(-3, 4, size=T).astype(np.float32)
    mem.dones[:] = 0.0
    mem.dones[T - 1] = 1.0
    mem.idx, mem.size = 0, T
    params = [p for g in model.optimizer.param_groups for p in g["params"]]
    lrs = [g["lr"] for g in model.optimizer.param_groups for _ in g["params"]]
    steps = []
    wrap_optimizer(model.optimizer, params, steps, torch)
    model.train_step()
    group = model.optimizer.param_groups[0]
    assert all(p.dtype == torch.float64 for p in params) and len(set(lrs)) == 2
    meta = dict(dtype="float64", tensors=len(params), steps=len(steps), lrs=lrs, betas=list(group["betas"]), eps=group["eps"], tau=None,
                max_norm=None, per_tensor=list(PER_TENSOR_PPO), per_step=["step"], shapes=[list(p.shape) for p in params])
    return meta, steps


def check(name, meta, steps):
    """The restatement, fed the reference's own coefficient, against the reference's results: the shares of the tolerances."""
    dtype = np.dtype(meta["dtype"])
    clipped = meta["max_norm"] is not None
    shares, exact = dict(param=0.0, norm=0.0), True
    for s, rec in enumerate(steps):
        assert int(rec["step"]) == s + 1
        coef = AC.torch_clip_coef(rec["norm"], meta["max_norm"], dtype) if clipped else None
        got = AC.restate(AC.fixture_tensors(rec, meta["lrs"], clipped), dtype, clip_mode=AC.CLIP_COEF if clipped else AC.CLIP_NONE, coef=coef,
                         beta1=meta["betas"][0], beta2=meta["betas"][1], eps=meta["eps"], tau=meta["tau"] or 0.0, step=s + 1)
        for k, t in enumerate(got["tensors"]):
            pairs = [("m", "exp_avg_after"), ("v", "exp_avg_sq_after")] + ([("t", "target_after")] if clipped else [])
            for mine, theirs in pairs:
                if not np.array_equal(AC.bits(t[mine]), AC.bits(rec[theirs][k])):
                    exact = False
                    print(f"{name} step {s} tensor {k}: {theirs} differs in {int((AC.bits(t[mine]) != AC.bits(rec[theirs][k])).sum())} elements")
            tol = AC.param_tolerance(rec["param_after"][k], rec["param_before"][k], dtype)
            err = np.abs(t["p"].astype(np.float64) - rec["param_after"][k].astype(np.float64))
            if err.size:
                shares["param"] = max(shares["param"], float(np.max(err / np.maximum(tol, 1e-300))))
            if clipped:
                assert np.array_equal(AC.bits(rec["grad"][k] * coef), AC.bits(rec["grad_clipped"][k])), "the coefficient is not torch's"
        if clipped:
            norm = AC.grad_norm(rec["grad"])
            n_total = sum(g.size for g in rec["grad"])
            shares["norm"] = max(shares["norm"], abs(norm - float(rec["norm"])) / AC.norm_tolerance(n_total, norm, dtype))
    print(f"{name}: share of the tolerance the reference uses: {shares}; moments and targets bit for bit: {exact}")
    assert max(shares.values()) <= 0.5, shares
    return shares, exact


def save(name, meta, steps):
    arrays = {}
    for s, rec in enumerate(steps):
        for key in meta["per_tensor"]:          # (one flat array per key and step: a zip entry per tensor would double the file)
            arrays[f"{key}_{s}"] = np.concatenate([a.reshape(-1) for a in rec[key]])
        for key in meta["per_step"]:
            arrays[f"{key}_{s}"] = np.asarray(rec[key])
    os.makedirs(AC.FIXTURE_DIR, exist_ok=True)
    path = os.path.join(AC.FIXTURE_DIR, name + ".npz")
    np.savez_compressed(path, params=json.dumps(meta), **arrays)
    print(f"{path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 200 * 1024


def main() -> None:
    ref_loader.install()
    import torch

    meta, steps = run_iqn(torch)
    norms = [float(s["norm"]) for s in steps]
    print("iqn: tensors", meta["tensors"], "numels", [int(np.prod(s)) for s in meta["shapes"]], "norms", norms)
    assert meta["tensors"] == 16 and len(steps) == 4 and any(int(np.prod(s)) == 1 for s in meta["shapes"])
    assert any(n > 1.0 for n in norms) and any(n < 1.0 for n in norms), norms
    meta["share"], meta["moments_exact"] = check("iqn", meta, steps)
    save("iqn", meta, steps)
    meta, steps = run_ppo(torch)
    assert len(steps) == 3
    meta["share"], meta["moments_exact"] = check("ppo", meta, steps)
    save("ppo", meta, steps)


if __name__ == "__main__":
    main()
