"""What the tests of the IQN learner (``sorrel_amd.models.PyTorchIQN``) share: the fixture of the reference's own ``iRainbowModel.train_step``
(``tests/golden/iqn_learner/train_steps.npz``, written by ``tools/make_iqn_learner_golden.py``), models put into a recorded state, and the
cap on a parameter's distance from the float64 step (DESIGN 0.19's form and factor)."""
import json
import os

import numpy as np

from tests import helpers as H

FIXTURE = os.path.join(H.ROOT, "tests", "golden", "iqn_learner", "train_steps.npz")
# (obs, n_frames, L, N, A, B)
SHAPES = ((9, 1, 7, 5, 3, 6), (7, 5, 17, 13, 5, 9))
STEPS = 3
SEED = 31
HYPER = dict(LR=0.001, TAU=0.001, GAMMA=0.99, n_step=3)          # the reference's defaults, which the fixture was made with
BATCH = ("states", "actions", "rewards", "next_states", "dones", "valid")


def tag_of(shape):
    return "_".join(str(v) for v in shape)


def cap(d_ref, p64):
    """``4 d_ref + 2^-22 max|p64|``"""
    p64 = np.asarray(p64, np.float64)
    return 4.0 * float(d_ref) + 2.0 ** -22 * (float(np.abs(p64).max()) if p64.size else 0.0)


def distance(p, p64):
    p, p64 = np.asarray(p, np.float64), np.asarray(p64, np.float64)
    return float(np.abs(p.reshape(p64.shape) - p64).max()) if p64.size else 0.0


_cache = {}


def load_fixture():
    """``{tag: dict(shape, sd_names, param_names, snaps, steps)}``.  ``snaps[k]`` is the state before step ``k`` (= after step ``k - 1``):
    ``local`` / ``target`` (name -> array of the ``state_dict``), ``exp_avg`` / ``exp_avg_sq`` (parameter name -> array; empty before step 0)
    and ``step``.  ``steps[k]``: ``batch`` (six arrays), ``taus`` (three ``[B, N, 1]``), ``eps`` (18 arrays), ``loss``, ``after64``
    (``local`` / ``target``: parameter name -> the float64 step's result) and ``d_ref`` (``local/<name>`` -> distance)."""
    if _cache:
        return _cache
    with np.load(FIXTURE) as data:
        arrays = {k: data[k] for k in data.files}
    meta = json.loads(str(arrays.pop("params")))
    for case in meta["cases"]:
        tag = case["tag"]
        snaps, steps = [], []
        for k in range(STEPS + 1):
            pre = f"{tag}/s{k}/"
            snap = dict(step=k, local={}, target={}, exp_avg={}, exp_avg_sq={})
            for key, value in arrays.items():
                if key.startswith(pre):
                    part, name = key[len(pre):].split("/", 1)
                    snap[part][name] = value
            snaps.append(snap)
        for k in range(STEPS):
            pre = f"{tag}/t{k}/"
            rec = dict(batch=tuple(arrays[pre + "batch/" + n] for n in BATCH), taus=[arrays[pre + f"taus/{c}"] for c in range(3)],
                       eps=[arrays[pre + f"eps/{i}"] for i in range(18)], loss=arrays[pre + "loss"], after64=dict(local={}, target={}),
                       d_ref=case["d_ref"][k])
            for key, value in arrays.items():
                if key.startswith(pre + "after64/"):
                    part, name = key[len(pre) + 8:].split("/", 1)
                    rec["after64"][part][name] = value
            steps.append(rec)
        _cache[tag] = dict(shape=tuple(case["shape"]), sd_names=case["sd_names"], param_names=case["param_names"], snaps=snaps, steps=steps)
    return _cache


def make_model(shape, device, seed=SEED, **kw):
    from sorrel_amd.models import PyTorchIQN

    obs, n_frames, L, N, A, B = shape
    args = dict(n_frames=n_frames, batch_size=B, memory_size=4 * B + 8 * n_frames, n_quantiles=N, **HYPER)
    args.update(kw)
    return PyTorchIQN((obs,), A, L, 0.0, device, seed, **args)


def fill_memory(model, rows=None, seed=0):
    """Random transitions (a done now and then) into every env of the model's ring, past the gate."""
    import torch

    mem = model.memory
    rows = mem.capacity - 2 if rows is None else rows
    g = torch.Generator().manual_seed(seed)
    E, dev = mem.num_envs, mem.device
    for t in range(rows):
        done = (torch.rand((E,), generator=g) < 0.1).float()
        mem.add(torch.randn((E,) + tuple(mem.obs_shape), generator=g).to(dev), torch.randint(0, model.action_space, (E,), generator=g).to(dev),
                torch.randn((E,), generator=g).to(dev), done.to(dev))
    return model


def put_state(model, snap):
    """The networks' ``state_dict``s and Adam's moments and step count of a recorded state."""
    import torch

    model.qnetwork_local.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in snap["local"].items()})
    model.qnetwork_target.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in snap["target"].items()})
    opt = model.optimizer
    names = [n for n, _ in model.qnetwork_local.named_parameters()]
    state = {}
    if snap["exp_avg"]:
        for i, n in enumerate(names):
            state[i] = dict(step=torch.tensor(float(snap["step"])), exp_avg=torch.from_numpy(np.array(snap["exp_avg"][n])),
                            exp_avg_sq=torch.from_numpy(np.array(snap["exp_avg_sq"][n])))
    opt.load_state_dict(dict(state=state, param_groups=opt.state_dict()["param_groups"]))
    model.steps_done = int(snap["step"])
    return model


def get_state(model):
    """The same, read back as NumPy arrays."""
    names = [n for n, _ in model.qnetwork_local.named_parameters()]
    st = model.optimizer.state_dict()["state"]
    return dict(local={k: v.detach().cpu().numpy().copy() for k, v in model.qnetwork_local.state_dict().items()},
                target={k: v.detach().cpu().numpy().copy() for k, v in model.qnetwork_target.state_dict().items()},
                exp_avg={n: st[i]["exp_avg"].cpu().numpy().copy() for i, n in enumerate(names) if i in st},
                exp_avg_sq={n: st[i]["exp_avg_sq"].cpu().numpy().copy() for i, n in enumerate(names) if i in st},
                step=int(st[0]["step"]) if 0 in st else 0)


def step_args(rec, device):
    """``train_step``'s keyword hooks of a recorded step, as tensors on ``device``."""
    import torch

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(device)

    B, N = rec["taus"][0].shape[:2]
    return dict(batch=tuple(dev(a) for a in rec["batch"]), taus=[dev(t.reshape(B, N)) for t in rec["taus"]], noise=[dev(e) for e in rec["eps"]])


def same_state(got, want, parts=("local", "target", "exp_avg", "exp_avg_sq"), ctx="", skip_epsilon=False):
    """Every tensor of two states in every bit (the epsilon buffers excepted on request: the device path keeps its noise elsewhere)."""
    from tests import learner_common as LK

    for part in parts:
        assert sorted(got[part]) == sorted(want[part]), (ctx, part)
        for name in want[part]:
            if skip_epsilon and "epsilon" in name:
                continue
            LK.same_bits(got[part][name], want[part][name], f"{part}/{name}", ctx)
    assert got["step"] == want["step"], ctx
