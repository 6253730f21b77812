"""TEST INFRASTRUCTURE ONLY -- generate ``tests/golden/iqn_backward/backward.npz`` from the reference's IQN network and torch's autograd.

Needs the reference checkout (``oracle/ref_loader.py``).  Usage::

    PYTHONDONTWRITEBYTECODE=1 python tools/make_iqn_backward_golden.py

What runs is the reference's own ``IQN`` (``sorrel/models/pytorch/iqn.py``) on the CPU: per small set of the forward's fixture once in eval
and once in train mode, ``calc_cos`` wrapped to keep ``cos`` and the taus, then ``(quantiles * grad_quantiles).sum().backward()`` for drawn
``grad_quantiles`` (one case one-hot in the action, as the loss makes it).  The same call is repeated by a float64 copy of the module
whose ``calc_cos`` hands back the kept values (``normal_`` is a no-op meanwhile: a noisy layer applies the float32 call's noise).  Stored per case:
the ``state_dict`` after the call, the inputs, and autograd's gradients of every parameter (sigmas included) in float32 and float64.  For
the reference's own shape (weights, states and taus of the forward's fixture, eval mode) only the float64 gradients are stored, rounded
to float32, and ``head1.weight``'s for every eighth row.  Data only.

The generator asserts the cap of ``tests/iqn_backward_common.py`` for the NumPy restatement per parameter tensor as it goes, and HALF of it
once the fixture is written (it lists the tensors between the two: a serial chain over the batch rows is a less accurate sum than torch's
blocked one, so the margin is thin where a gradient is a long sum of like-signed terms, the biases').  It writes both
distances (``d_ref``: the reference's float32 against float64; ``d_r``: the restatement's) into the fixture and prints them as the table
of DESIGN.md."""
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
from tests import iqn_backward_common as BC  # noqa: E402
from tests import iqn_forward_common as FC  # noqa: E402

OUT = BC.FIXTURE
MISSED_HALF = []                              # tensors whose restatement holds the cap but not half of it: the last assertion of main()


class pinned_noise:
    """While it is open, ``Tensor.normal_`` leaves a tensor as it is: a noisy layer (which draws new noise per call) applies the epsilon
    it holds."""

    def __init__(self, torch):
        self.torch = torch

    def __enter__(self):
        self.real = self.torch.Tensor.normal_
        self.torch.Tensor.normal_ = lambda t, *a, **k: t

    def __exit__(self, *exc):
        self.torch.Tensor.normal_ = self.real


def run(layers_mod, torch, net, states, N, train, grad, given=None):
    """One forward + backward of the reference's module: ``(cos, taus, {parameter: gradient})``."""
    seen = {}
    real = net.calc_cos

    def calc_cos(batch_size, n_tau=8):
        if given is not None:
            return given
        cos, taus = real(batch_size, n_tau)
        seen["cos"], seen["taus"] = cos.detach().clone(), taus.detach().clone()
        return cos, taus

    net.train(train)
    net.zero_grad()
    net.calc_cos = calc_cos
    try:
        quant, taus = net(states, N)
    finally:
        del net.calc_cos
    (quant * grad).sum().backward()
    cos, taus = given if given is not None else (seen["cos"], seen["taus"])
    return cos, taus, {k: p.grad.detach().numpy().copy() for k, p in net.named_parameters() if p.grad is not None}


def case_of(layers_mod, torch, net, states, N, train, grad, given=None):
    cos, taus, g32 = run(layers_mod, torch, net, torch.from_numpy(states), N, train, torch.from_numpy(grad), given)
    sd = {k: v.numpy().copy() for k, v in net.state_dict().items()}
    net64 = copy.deepcopy(net).double()
    with pinned_noise(torch):
        _, _, g64 = run(layers_mod, torch, net64, torch.from_numpy(states).double(), N, train, torch.from_numpy(grad).double(), (cos.double(), taus.double()))
    assert sorted(g32) == sorted(g64)
    for layer in ("ff_1", "advantage", "value"):                                  # the float64 call used the float32 call's noise
        assert np.array_equal(net64.state_dict()[f"{layer}.epsilon_weight"].numpy().astype(np.float32), sd[f"{layer}.epsilon_weight"])
    return sd, cos.numpy().copy(), taus.numpy().copy(), g32, g64


def distances(tag, sd, train, states, cos, grad, g32, g64, big=False):
    """Per parameter tensor ``(d_ref, d_r)``; asserts half of the cap for the restatement."""
    gw = BC.restate(FC.effective_of(sd, train), states, cos, grad)
    mine = BC.parameter_grads(gw, sd, train)
    assert sorted(mine) == sorted(g64), (sorted(mine), sorted(g64))
    d_ref, d_r = {}, {}
    for k in sorted(g64):
        d_ref[k], d_r[k] = BC.distance(g32[k], g64[k]), BC.distance(mine[k], g64[k])
        limit = BC.cap(d_ref[k], g64[k])
        print(f"| {tag} | {k} | {d_ref[k]:.3e} | {d_r[k]:.3e} | {limit:.3e} |")
        assert d_r[k] <= limit, f"{tag} {k}: the restatement lies {d_r[k]} from float64, the cap is {limit}"
        if d_r[k] > 0.5 * limit:
            MISSED_HALF.append(f"{tag} {k}: the restatement lies {d_r[k]:.4e} from float64, half the cap is {0.5 * limit:.4e}")
    return d_ref, d_r


def main() -> None:
    ref_loader.install()
    import torch
    from sorrel.models.pytorch import iqn, layers

    torch.set_num_threads(1)
    arrays, meta = {}, dict(cases=[])
    print("| case | parameter | d_ref | d_r | cap |\n|---|---|---|---|---|")
    for i, (D, L, N, A, B) in enumerate(BC.SMALL_SETS):
        for train in (False, True):
            tag = f"{D}_{L}_{N}_{A}_{B}/{'train' if train else 'eval'}"
            net = iqn.IQN((D,), A, L, seed=71 + i, n_quantiles=N, n_frames=1, device="cpu")
            rng = np.random.default_rng(71 + 2 * i + train)
            states = rng.normal(0.0, 1.0, size=(B, D)).astype(np.float32)
            grad = rng.normal(0.0, 1.0, size=(B, N, A)).astype(np.float32)
            one_hot = bool(train and i == 1)
            if one_hot:                                                          # as the loss makes it: the taken action's column alone
                keep = np.zeros((B, 1, A), np.float32)
                keep[np.arange(B), 0, rng.integers(0, A, size=B)] = 1.0
                grad = grad * keep
            sd, cos, taus, g32, g64 = case_of(layers, torch, net, states, N, train, grad)
            d_ref, d_r = distances(tag, sd, train, states, cos, grad, g32, g64)
            for k, v in sd.items():
                arrays[f"{tag}/sd/{k}"] = v
            arrays[f"{tag}/states"], arrays[f"{tag}/taus"], arrays[f"{tag}/cos"], arrays[f"{tag}/grad"] = states, taus, cos, grad
            for k in g32:
                arrays[f"{tag}/g32/{k}"], arrays[f"{tag}/g64/{k}"] = g32[k], g64[k]
            meta["cases"].append(dict(case=tag, big=False, train=train, one_hot=one_hot, D=D, L=L, N=N, A=A, B=B, sd_keys=sorted(sd),
                                      grad_keys=sorted(g32), d_ref=d_ref, d_r=d_r))
    # the reference's own shape: weights, states and taus of the forward's fixture
    s = FC.load_fixture()[BC.BIG_TAG]
    D, L, N, A, B = (s[k] for k in "DLNAB")
    net = iqn.IQN((D,), A, L, seed=0, n_quantiles=N, n_frames=1, device="cpu")
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in s["sd"].items()})
    rng = np.random.default_rng(79)
    grad = rng.normal(0.0, 1.0, size=(B, N, A)).astype(np.float32)
    given = (torch.from_numpy(s["eval"]["cos"]), torch.from_numpy(s["eval"]["taus"]))
    sd, cos, taus, g32, g64 = case_of(layers, torch, net, s["states"], N, False, grad, given)
    assert np.array_equal(cos, s["eval"]["cos"]) and all(np.array_equal(sd[k], s["sd"][k]) for k in sd)
    tag = BC.BIG_TAG + "/eval"
    d_ref, d_r = distances(tag, sd, False, s["states"], cos, grad, g32, g64)
    arrays[f"{tag}/grad"] = grad
    for k in g64:
        part = g64[k][BC.BIG_HEAD_ROWS] if k == "head1.weight" else g64[k]
        arrays[f"{tag}/g64/{k}"] = part.astype(np.float32)
    meta["cases"].append(dict(case=tag, big=True, set=BC.BIG_TAG, train=False, one_hot=False, D=D, L=L, N=N, A=A, B=B, grad_keys=sorted(g64),
                              d_ref=d_ref, d_r=d_r))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, params=json.dumps(meta), **arrays)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes (the forward's fixture: {os.path.getsize(FC.FIXTURE)})")
    assert os.path.getsize(OUT) < os.path.getsize(FC.FIXTURE)
    assert not MISSED_HALF, "the fixture is written and every tensor holds the cap, but not half of it:\n" + "\n".join(MISSED_HALF)


if __name__ == "__main__":
    main()
