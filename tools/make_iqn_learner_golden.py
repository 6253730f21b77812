"""TEST INFRASTRUCTURE ONLY -- generate ``tests/golden/iqn_learner/train_steps.npz`` from the reference's own learner.

Needs the reference checkout (``oracle/ref_loader.py``).  Usage::

    PYTHONDONTWRITEBYTECODE=1 python tools/make_iqn_learner_golden.py

What runs is the reference's ``iRainbowModel`` (``sorrel/models/pytorch/iqn.py``) on the CPU: per shape of ``tests/iqn_learner_common.py`` a
model over a filled replay buffer takes three consecutive ``train_step``s.  ``Buffer.sample``, ``IQN.calc_cos`` and ``NoisyLinear.forward``
are wrapped to keep what they drew: the batch, the three tau tensors and the 18 eps tensors of each step.  Stored per step: those, the
loss, and the state around it (both ``state_dict``s, Adam's ``exp_avg`` / ``exp_avg_sq`` and step count: the state after step k is the
state before step k + 1, stored once).  The same step is repeated from the same before-state by a float64 copy of the model that is handed
the kept batch, taus and noise; its parameters afterwards are stored in float64, and per parameter tensor ``d_ref``, the float32 step's
distance from them.  Data only.

The generator ends on two assertions about this repository's torch path (``PyTorchIQN.train_step(batch=, taus=, noise=)`` on the CPU, each
step started from its recorded before-state): it holds HALF of the cap ``4 d_ref + 2^-22 max|p64|`` for every parameter tensor (any tensor
between half and whole is listed), and it reproduces the reference's loss and after-state bit for bit."""
from __future__ import annotations

import copy
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_loader  # noqa: E402
from tests import iqn_learner_common as LC  # noqa: E402

OUT = LC.FIXTURE
FORWARD_FIXTURE = os.path.join(ROOT, "tests", "golden", "iqn_forward", "forward.npz")


class Recorder:
    """Wraps the three sources of randomness of a ``train_step``: records what they draw, or (``given``) hands back what was recorded."""

    def __init__(self, torch, iqn, layers, model, given=None, dtype=None):
        self.torch, self.iqn, self.layers, self.model, self.given, self.dtype = torch, iqn, layers, model, given, dtype
        self.batch, self.taus, self.eps = None, [], []

    def __enter__(self):
        torch, rec = self.torch, self
        self.real_sample = self.model.memory.sample
        self.real_cos = self.iqn.IQN.calc_cos
        self.real_forward = self.layers.NoisyLinear.forward
        self.real_normal = torch.Tensor.normal_

        def sample(batch_size):
            if rec.given is not None:
                return tuple(a.astype(np.float64) if a.dtype.kind == "f" else a for a in rec.given["batch"])
            rec.batch = tuple(np.array(a) for a in rec.real_sample(batch_size=batch_size))
            return rec.batch

        def calc_cos(net, batch_size, n_tau=8):
            if rec.given is not None:
                taus = torch.from_numpy(rec.given["taus"][len(rec.taus)]).to(rec.dtype)
                rec.taus.append(taus)
                return torch.cos(taus * net.pis), taus
            cos, taus = rec.real_cos(net, batch_size, n_tau)
            rec.taus.append(taus.detach().numpy().copy())
            return cos, taus

        def forward(layer, input):
            if rec.given is not None:
                k = len(rec.eps)
                layer.epsilon_weight.copy_(torch.from_numpy(rec.given["eps"][k]))
                layer.epsilon_bias.copy_(torch.from_numpy(rec.given["eps"][k + 1]))
                rec.eps += [None, None]
                torch.Tensor.normal_ = lambda t, *a, **kw: t              # the layer applies the epsilon it holds
                try:
                    return rec.real_forward(layer, input)
                finally:
                    torch.Tensor.normal_ = rec.real_normal
            out = rec.real_forward(layer, input)
            rec.eps += [layer.epsilon_weight.detach().numpy().copy(), layer.epsilon_bias.detach().numpy().copy()]
            return out

        self.model.memory.sample = sample
        self.iqn.IQN.calc_cos = calc_cos
        self.layers.NoisyLinear.forward = forward
        return self

    def __exit__(self, *exc):
        del self.model.memory.sample
        self.iqn.IQN.calc_cos = self.real_cos
        self.layers.NoisyLinear.forward = self.real_forward
        self.torch.Tensor.normal_ = self.real_normal


def snapshot(model):
    names = [n for n, _ in model.qnetwork_local.named_parameters()]
    st = model.optimizer.state_dict()["state"]
    return dict(local={k: v.detach().numpy().copy() for k, v in model.qnetwork_local.state_dict().items()},
                target={k: v.detach().numpy().copy() for k, v in model.qnetwork_target.state_dict().items()},
                exp_avg={n: st[i]["exp_avg"].numpy().copy() for i, n in enumerate(names) if i in st},
                exp_avg_sq={n: st[i]["exp_avg_sq"].numpy().copy() for i, n in enumerate(names) if i in st},
                step=int(st[0]["step"]) if 0 in st else 0)


def to_float64(torch, model):
    """A float64 copy of the reference's learner: both networks, their ``pis`` and Adam's moments."""
    m = copy.deepcopy(model)
    for net in (m.qnetwork_local, m.qnetwork_target):
        net.double()
        net.pis = net.pis.double()
    for st in m.optimizer.state.values():
        st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"].double(), st["exp_avg_sq"].double()
    return m


def main() -> None:
    ref_loader.install()
    import torch
    from sorrel.models.pytorch import iqn, layers

    torch.set_num_threads(1)
    arrays, meta = {}, dict(cases=[])
    for shape in LC.SHAPES:
        obs, n_frames, L, N, A, B = shape
        tag = LC.tag_of(shape)
        np.random.seed(LC.SEED)
        model = iqn.iRainbowModel((obs,), A, L, 0.0, "cpu", LC.SEED, n_frames=n_frames, batch_size=B, memory_size=4 * B + 8 * n_frames, n_quantiles=N,
                                  **LC.HYPER)
        rng = np.random.default_rng(LC.SEED)
        for _ in range(model.memory.capacity - 2):
            model.memory.add(rng.normal(size=(obs,)).astype(np.float32), int(rng.integers(0, A)), float(rng.normal()), bool(rng.random() < 0.1))
        assert len(model.memory) > B
        sd_names = list(model.qnetwork_local.state_dict())
        param_names = [n for n, _ in model.qnetwork_local.named_parameters()]
        snaps, d_refs = [snapshot(model)], []
        for k in range(LC.STEPS):
            model64 = to_float64(torch, model)
            with Recorder(torch, iqn, layers, model) as rec:
                loss = model.train_step()
            assert len(rec.taus) == 3 and len(rec.eps) == 18 and rec.batch is not None
            given = dict(batch=rec.batch, taus=rec.taus, eps=rec.eps)
            with Recorder(torch, iqn, layers, model64, given=given, dtype=torch.float64):
                loss64 = model64.train_step()
            assert abs(float(loss64) - float(loss)) <= 1e-5 * max(1.0, abs(float(loss64))), (float(loss), float(loss64))
            snaps.append(snapshot(model))
            pre = f"{tag}/t{k}/"
            for name, a in zip(LC.BATCH, rec.batch):
                arrays[pre + "batch/" + name] = a
            for c, t in enumerate(rec.taus):
                arrays[pre + f"taus/{c}"] = t
            for i, e in enumerate(rec.eps):
                arrays[pre + f"eps/{i}"] = e
            arrays[pre + "loss"] = np.asarray(loss)
            d_ref = {}
            for part, net in (("local", model64.qnetwork_local), ("target", model64.qnetwork_target)):
                for name, p in net.named_parameters():
                    p64 = p.detach().numpy().copy()
                    assert p64.dtype == np.float64
                    arrays[pre + f"after64/{part}/{name}"] = p64
                    d_ref[f"{part}/{name}"] = LC.distance(snaps[-1][part][name], p64)
            d_refs.append(d_ref)
        for k, snap in enumerate(snaps):
            assert snap["step"] == k
            for part in ("local", "target", "exp_avg", "exp_avg_sq"):
                for name, a in snap[part].items():
                    arrays[f"{tag}/s{k}/{part}/{name}"] = a
        meta["cases"].append(dict(tag=tag, shape=list(shape), sd_names=sd_names, param_names=param_names, d_ref=d_refs))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, params=json.dumps(meta), **arrays)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes (the forward's fixture: {os.path.getsize(FORWARD_FIXTURE)})")
    assert os.path.getsize(OUT) < os.path.getsize(FORWARD_FIXTURE)

    # this repository's torch path against the fixture just written
    from tests import learner_common as LK

    LC._cache.clear()
    missed_half, differ = [], []
    print("| shape | step | tensor | d_ref | d_r (torch path) | cap |\n|---|---|---|---|---|---|")
    for tag, case in LC.load_fixture().items():
        for k, rec in enumerate(case["steps"]):
            mine = LC.put_state(LC.make_model(case["shape"], "cpu"), case["snaps"][k])
            LC.fill_memory(mine)
            loss = mine.train_step(**LC.step_args(rec, "cpu"))
            got, want = LC.get_state(mine), case["snaps"][k + 1]
            if not (np.asarray(loss).dtype == rec["loss"].dtype and LK.bits(np.asarray(loss)) == LK.bits(rec["loss"])):
                differ.append(f"{tag} step {k}: loss {loss!r} != {rec['loss']!r}")
            for part in ("local", "target"):
                for name in case["param_names"]:
                    p64 = rec["after64"][part][name]
                    d_ref, d_r = rec["d_ref"][f"{part}/{name}"], LC.distance(got[part][name], p64)
                    limit = LC.cap(d_ref, p64)
                    print(f"| {tag} | {k} | {part}/{name} | {d_ref:.3e} | {d_r:.3e} | {limit:.3e} |")
                    assert d_r <= limit, f"{tag} step {k} {part}/{name}: the torch path lies {d_r} from float64, the cap is {limit}"
                    if d_r > 0.5 * limit:
                        missed_half.append(f"{tag} step {k} {part}/{name}: {d_r:.4e} from float64, half the cap is {0.5 * limit:.4e}")
            for part in ("local", "target", "exp_avg", "exp_avg_sq"):
                for name, a in want[part].items():
                    if not np.array_equal(LK.bits(got[part][name]), LK.bits(a)):
                        differ.append(f"{tag} step {k}: {part}/{name} differs in {int((LK.bits(got[part][name]) != LK.bits(a)).sum())} of {a.size} elements")
    assert not missed_half, "every tensor holds the cap, but not half of it:\n" + "\n".join(missed_half)
    assert not differ, "the torch path does not reproduce the reference bit for bit:\n" + "\n".join(differ)


if __name__ == "__main__":
    main()
